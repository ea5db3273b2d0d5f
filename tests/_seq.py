"""Model-based sequences of group and batch operations (tests/test_gpu_state_sequences.py, tests/test_state_sequences_cpu.py).

One long-lived resident group with two or three batches is taken through a seeded random interleaving of appends, staged commits,
gathers, slides, fused slide-and-score calls, window settings, screened and plain Runs, many-reference passes, cache builds and
drops and Muse.Runs off a template: the way a host that follows time drives the library.  Three parts:

  Model      what the rows must be (a float64 numpy array; through np.float32 for a float32-storage group), every batch's window,
             the engine-wide switches in force -- numpy and plain Python only
  generate   the operation list of a (class, seed): every operation has a weight and a precondition, everything is drawn from
             np.random.default_rng(seed); no device, no library
  Runner     applies the operations to the device and to the model side by side and checks every result

Expected values never come from the code under test: rows are compared byte for byte with the model; all-scores passes with
oracle.batch_scores (no window) or the lag-window definition of tests/_window.py applied to the oracle's correlation (a window) on the
MODEL's rows, by the project's rules (scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact off the oracle's ties,
ties at most 1 in 1000 continuous-noise rows); Runs with oracle.results fed the per-row (lag, mv) the same batch's all-scores pass
returned for the same state (that pass has itself just been held to the oracle: tests/test_gpu_parity.py,
test_fuzz_run_semantics_against_oracle).  The comparison helpers are the suite's own (check of test_gpu_lag_window.py,
assert_scores_match of test_gpu_parity.py, winner / assert_winner of test_gpu_window_rows.py), imported from where they are.

Rows: the noise + shifted-reference mix of _window.make_case, per appended chunk, with its constant, NaN, Inf and mean-1e6 rows and
its exact copy / negated copy of the reference.  One difference, on purpose: at most ONE row whose |score| is 1 exists at a time
(a chunk plants the copy or the negated copy, in turn, only when no such row is left) -- a screened Run re-evaluates its candidates
with another fp64 kernel whose scores differ from the all-scores pass's in the last bits (test_gpu_parity.py: 1e-12 / 5e-11), and
two rows at |score| = 1 +- rounding would make the order of a Run's first two results a matter of those bits.

A failing step prints the seed, the step and the operation list so far as a call that can be pasted back: replay(...).
MUSE_TEST_SEQ_SEED=<int> adds one more seed to every parametrisation."""
import hashlib
import json
import math
import os

import numpy as np

import _window as W

WINDOWS = (-1, 0, 7, 15, 16, 63)
STAGE_SLAB_BYTES = 8 << 20       # muse_group_append uploads a piece of at least this size directly (capi_group.hip: STAGE_BYTES / 4)
SRC_ROWS = 24                    # rows of the second resident group the gathers read

# shape classes: the smallest shapes that still reach the state in question (the issue's table)
CLASSES = {
    "a": dict(N=4096, f32=False, M0=200, steps=50, cache=True),       # fold kernel, spectrum cache and its segments, cached reader
    "b": dict(N=480, f32=False, M0=150, steps=40),                    # small kernel, small-Run path, packed appends
    "c": dict(N=1433, f32=False, M0=100, steps=40),                   # odd N: narrow window mapping, 8-byte slide unit, padded n = 2048
    "d": dict(N=5000, f32=False, M0=60, steps=40),                    # real-transform n = 8192 kernel, padded
    "e": dict(N=480, f32=True, M0=100, steps=40),                     # 4-byte slide unit, window refusals
    "f": dict(N=70000, f32=False, M0=6, steps=26),                    # kept statistics of the huge path across slides and appends
    "g": dict(N=4096, f32=False, M0=2100, steps=12, cache=True, scale30=True, wcap=1, window_setting=False),  # dense hand-off list
}
# two seeds per class, chosen so that the coverage conditions of tests/test_state_sequences_cpu.py hold
SEEDS = {"a": (20, 42), "b": (22, 24), "c": (4, 33), "d": (28, 52), "e": (1, 8), "f": (20, 43), "g": (1, 16)}


def seeds_of(cls):
    extra = os.environ.get("MUSE_TEST_SEQ_SEED")
    return tuple(SEEDS[cls]) + ((int(extra),) if extra else ())


class Shape:
    def __init__(self, cls):
        c = CLASSES[cls]
        self.cls, self.N, self.f32, self.M0, self.steps = cls, c["N"], c["f32"], c["M0"], c["steps"]
        self.n = 1 << max(0, (self.N - 1).bit_length())
        self.cache = bool(c.get("cache"))
        self.scale30 = bool(c.get("scale30"))
        self.wcap = c.get("wcap", 10 ** 9)                             # windowed readers a sequence may hold (the CPU oracle is the cost)
        self.window_ok = not self.f32 and self.n <= 65536              # muse_batch_set_lag_window's own limits
        self.window_setting = self.window_ok and c.get("window_setting", True)
        self.stage_ok = not self.f32                                   # staging windows hold float64 rows
        self.screen_ok = not self.f32 and 512 <= self.n <= 65536       # screen_path's length_ok
        self.slab = -(-STAGE_SLAB_BYTES // (8 * self.N)) if not self.f32 else 300   # (float32 groups pack every append)


# ------------------------------------------------------------------ operation kinds
MUTATORS = ("append", "stage_commit", "append_from", "slide", "slide_score", "slide_run", "drop_cache", "trim")
SETTINGS = ("window", "screening", "cache_limits", "reuse")
READERS = ("scores", "run", "run_groups", "scores_many", "run_many", "scores_many_w", "run_many_w", "run_group_rows", "run_rows",
           "run_rows_w", "muse_run", "read")
REFUSALS = ("refuse_window_f32", "refuse_windowed_template", "refuse_slide_score_window", "refuse_slide_staged", "refuse_slide_k")
GROUP = dict([(k, "mutator") for k in MUTATORS] + [(k, "setting") for k in SETTINGS] + [(k, "reader") for k in READERS] +
             [(k, "refusal") for k in REFUSALS])
# the kinds the coverage condition counts: the bullets of the operation list
FAMILY = dict(append="append", stage_commit="stage_commit", append_from="append_from", slide="slide", slide_score="slide_score",
              slide_run="slide_score", drop_cache="drop_cache", trim="trim", window="window", screening="screening",
              cache_limits="cache_limits", reuse="reuse", scores="scores", run="run", run_groups="run_groups", scores_many="many",
              run_many="many", scores_many_w="many", run_many_w="many", run_group_rows="template", run_rows="template",
              run_rows_w="template", muse_run="template", read="read")
READER_FAMILIES = ("scores", "run", "run_groups", "many", "template", "read")
WEIGHT = dict(append=3, stage_commit=2, append_from=2, slide=4, slide_score=3, slide_run=2, drop_cache=2, trim=1, window=3, screening=2,
              cache_limits=1, reuse=1, scores=4, run=4, run_groups=2, scores_many=2, run_many=2, scores_many_w=2, run_many_w=2,
              run_group_rows=2, run_rows=1, run_rows_w=1, muse_run=1, read=1)


def stored(x, f32):
    """what a group of that storage type holds for the float64 samples x"""
    with np.errstate(all="ignore"):
        return x.astype(np.float32).astype(np.float64) if f32 else np.array(x, dtype=np.float64)


def slide_ks(N):
    return sorted({min(k, N) for k in (1, 2, 3, 16, 65, N // 2, N)})


# ------------------------------------------------------------------ the model
class Model:
    def __init__(self, cls, seed):
        self.shape = s = Shape(cls)
        self.seed = int(seed)
        rng = np.random.default_rng([self.seed, ord(cls), 0x5E9])
        N = s.N
        self.R = int(rng.integers(2, 4))
        w = max(1, N // 20)
        self.refs = []
        for j in range(self.R):                                        # _window.make_case's reference; the others: the pulse moved a little
            ref = np.zeros(N)
            ref[N // 2 - w // 2:N // 2 - w // 2 + w] = 2.0
            self.refs.append(np.roll(ref, 5 * j) + 0.1 * rng.standard_normal(N))
        self.rows = np.zeros((0, N))
        self.kinds = []
        self.version = 0                                               # bumps whenever the rows change
        self.slides = 0
        self.windows = [-1] * self.R
        self.packed = [False] * self.R                                 # the batch's scores come from a packed many-references launch
        self.screening = False
        self.reuse = True
        self.cache_limits = False
        self.slab_done = False
        self.next_sign = 1
        self.wreads = 0
        self.src_rows, self.src_kinds = self._chunk(SRC_ROWS, int(rng.integers(1 << 30)), base=1, unit_row=False)
        self.src_rows = stored(self.src_rows, s.f32)
        self.initial_raw, kinds = self._chunk(s.M0, int(rng.integers(1 << 30)))
        self._extend(self.initial_raw, kinds)
        self.version = 0

    @property
    def M(self):
        return self.rows.shape[0]

    def keep(self):
        """the continuous-noise rows (the cap on tied rows counts them)"""
        return np.array([k in ("plain", "mean") for k in self.kinds], dtype=bool)

    def _chunk(self, count, dseed, base=None, unit_row=True):
        """`count` rows as _window.make_case draws them (row classes by global row index), specials planted from 8 rows on"""
        s = self.shape
        N, ref = s.N, self.refs[0]
        rng = np.random.default_rng([int(dseed), 0xC4])
        base = len(self.kinds) if base is None else base
        rows = np.zeros((count, N))
        kinds = ["plain"] * count
        far_lo, far_hi = (64, max(65, min(N // 4, 500)))
        for r in range(count):
            c = (base + r) % 3
            if c == 0:
                shift, noise = 0, 0.02
            elif c == 1:
                shift, noise = int(rng.integers(far_lo, far_hi + 1)) * (1 if rng.random() < 0.5 else -1), 0.3
            else:
                shift, noise = int(rng.integers(-70, 71)), 0.3
            rows[r] = (0.5 + rng.random()) * np.roll(ref, shift) + noise * rng.standard_normal(N) + rng.standard_normal()
        if count >= 8:
            if unit_row and not any(k in ("copy", "neg") for k in self.kinds):
                rows[1] = self.next_sign * ref
                kinds[1] = "copy" if self.next_sign > 0 else "neg"
                self.next_sign = -self.next_sign
            rows[3] = 3.25
            kinds[3] = "const"
            rows[4] = rows[0]
            rows[4, N // 3] = np.nan
            kinds[4] = "nan"
            rows[5] = rows[0]
            rows[5, N // 2] = np.inf
            kinds[5] = "inf"
            z = rng.standard_normal(N)
            rows[6] = 1e6 + (z - z.mean()) / z.std()
            kinds[6] = "mean"
        if s.scale30:                                                  # mixed units: every other row x 1e30
            rows[(base + np.arange(count)) % 2 == 1] *= 1e30
        return rows, kinds

    def _tails(self, first, count, k, dseed):
        """the next k samples of rows [first, first + count): noise around each row's own mean at its own spread; a constant row stays
        constant, a NaN / Inf row keeps one"""
        rng = np.random.default_rng([int(dseed), 0x7A])
        cur = self.rows[first:first + count]
        with np.errstate(all="ignore"):
            fin = np.isfinite(cur)
            cnt = np.maximum(fin.sum(1), 1)
            mean = np.where(fin, cur, 0.0).sum(1) / cnt
            sd = np.sqrt((np.where(fin, cur - mean[:, None], 0.0) ** 2).sum(1) / cnt)
            t = mean[:, None] + sd[:, None] * rng.standard_normal((count, k))
        for i, kind in enumerate(self.kinds[first:first + count]):
            if kind == "const":
                t[i, :] = cur[i, -1]
            elif kind == "nan":
                t[i, 0] = np.nan
            elif kind == "inf":
                t[i, 0] = np.inf
        return t

    def _extend(self, raw, kinds):
        self.rows = np.vstack([self.rows, stored(raw, self.shape.f32)])
        self.kinds = self.kinds + list(kinds)
        self.version += 1

    def _slide(self, first, tails):
        count, k = tails.shape
        cur = self.rows[first:first + count]
        self.rows = self.rows.copy()
        self.rows[first:first + count] = np.concatenate([cur[:, k:], stored(tails, self.shape.f32)], 1)
        for r in range(first, first + count):
            if self.kinds[r] in ("copy", "neg"):
                self.kinds[r] = "plain"
        self.version += 1
        self.slides += 1

    # ---- preconditions (what the library's own documentation requires of the call; the refusals: what makes it refuse)
    def windowed_reader(self, op):
        """does this operation need a windowed expectation (one oracle transform per row in Python: class g allows one)"""
        k = op["kind"]
        if k in ("scores", "run", "run_groups"):
            return self.windows[op["j"]] >= 0
        return k in ("scores_many_w", "run_many_w", "run_rows_w", "slide_score", "slide_run")

    def precondition(self, op):
        s, k = self.shape, op["kind"]
        if self.windowed_reader(op) and (not s.window_ok or self.wreads >= s.wcap):
            return False
        if k == "append":
            return op["count"] >= 1 and (op["how"] != "slab" or not self.slab_done)
        if k == "stage_commit":
            return s.stage_ok and sorted(r for f, c in op["pieces"] for r in range(f, f + c)) == list(range(op["count"]))
        if k == "append_from":
            return len(op["idx"]) >= 1 and all(0 <= i < SRC_ROWS for i in op["idx"])
        if k == "slide":
            return op["count"] >= 1 and 0 <= op["first"] and op["first"] + op["count"] <= self.M and 1 <= op["k"] <= s.N
        if k in ("slide_score", "slide_run"):
            return self.M >= 1 and 1 <= op["k"] <= s.N and 0 <= op["L"] <= 63 and self.windows[op["j"]] in (-1, op["L"])
        if k in ("drop_cache", "cache_limits"):
            return s.cache
        if k == "window":
            return s.window_setting and op["L"] in WINDOWS and op["L"] != self.windows[op["j"]]
        if k in ("trim", "screening", "reuse", "read", "scores", "run", "run_groups"):
            return self.M >= 1
        if k in ("scores_many", "run_many"):
            return len(op["js"]) >= 1 and all(self.windows[j] < 0 for j in op["js"])
        if k in ("scores_many_w", "run_many_w"):
            return len(op["js"]) >= 1 and all(self.windows[j] in (-1, op["L"]) for j in op["js"])
        if k in ("run_group_rows", "run_rows", "run_rows_w"):
            top = SRC_ROWS if op.get("src") == "src" else self.M
            return len(op["idx"]) >= 1 and all(0 <= i < top for i in op["idx"])
        if k == "muse_run":
            return len(op["idx"]) >= 1 and all(0 <= i < s.M0 for i in op["idx"])
        if k == "refuse_window_f32":
            return s.f32 and op["L"] >= 0
        if k == "refuse_windowed_template":
            return self.windows[op["j"]] >= 0
        if k == "refuse_slide_score_window":
            return s.window_ok and self.windows[op["j"]] >= 0 and op["L"] >= 0 and op["L"] != self.windows[op["j"]]
        if k == "refuse_slide_staged":
            return s.stage_ok and self.M >= 1 and op["count"] >= 1
        if k == "refuse_slide_k":
            return self.M >= 1
        raise KeyError(k)

    # ---- the arrays an operation hands to the device, from the state in front of it
    def prepare(self, op):
        k = op["kind"]
        d = {}
        if k in ("append", "stage_commit", "refuse_slide_staged"):
            d["rows"], d["kinds"] = self._chunk(op["count"], op["dseed"])
        elif k == "append_from":
            idx = np.array(op["idx"], dtype=np.int64)
            d["rows"], d["kinds"] = self.src_rows[idx], [self.src_kinds[i] for i in idx]
        elif k == "slide":
            d["tails"] = self._tails(op["first"], op["count"], op["k"], op["dseed"])
        elif k in ("slide_score", "slide_run", "refuse_slide_score_window"):
            d["tails"] = self._tails(0, self.M, op["k"], op["dseed"])
        if "G" in op:
            G = op["G"]
            d["gid"] = None if G == 0 else np.random.default_rng([int(op["gseed"]), 0x91]).integers(0, G, size=self.M).astype(np.int32)
        return d

    def apply(self, op, d):
        k = op["kind"]
        if self.windowed_reader(op):
            self.wreads += 1
        if k in ("append", "stage_commit", "append_from", "refuse_slide_staged"):
            self._extend(d["rows"], d["kinds"])
            if k == "append" and op["how"] == "slab":
                self.slab_done = True
        elif k == "slide":
            self._slide(op["first"], d["tails"])
        elif k in ("slide_score", "slide_run"):
            self._slide(0, d["tails"])
            self.packed[op["j"]] = False
        elif k == "window":
            self.windows[op["j"]] = op["L"]
        elif k == "screening":
            self.screening = bool(op["on"])
        elif k == "reuse":
            self.reuse = bool(op["on"])
        elif k == "cache_limits":
            self.cache_limits = bool(op["on"])
        elif k in ("scores", "run", "run_groups"):
            self.packed[op["j"]] = False
        elif k in ("scores_many", "run_many"):
            for j in op["js"]:
                self.packed[j] = False
        # (scores_many_w / run_many_w: which references share a launch is the planner's word -- the runner sets `packed`)

    def screen_eligible(self, op):
        """screen_path's own conditions, from the model: may this Run take the filter-and-refine path"""
        return self.screening and self.shape.screen_ok and self.windows[op["j"]] < 0 and 1 <= op["top_n"] <= 256 and self.M >= 2


# ------------------------------------------------------------------ the generator
def _run_params(m, rng, screened=False):
    N, M = m.shape.N, m.M
    if rng.random() < 0.25:
        G = 0
    else:
        G = int(rng.integers(1, max(2, 2 * M)))
    return dict(G=G, gseed=int(rng.integers(1 << 30)), max_lag=int(rng.choice([0, 3, 15, N // 4, N])),
                top_n=int(rng.choice([1, 5, 20] if screened else [1, 5, 20, 257])), thr=float(rng.choice([0.0, 0.05, 0.3])),
                sign=int(rng.choice([0, 1, -1])), abs=bool(rng.random() < 0.6))


def _idx(rng, top, lo=2, hi=20, distinct=True):
    count = int(rng.integers(lo, min(hi, top) + 1)) if top >= lo else top
    if rng.random() < 0.4:                                             # one ascending run: scored where it lies
        first = int(rng.integers(0, top - count + 1))
        return list(range(first, first + count))
    idx = [int(i) for i in rng.integers(0, top, size=count)]
    return list(dict.fromkeys(idx)) if distinct else idx              # (a row listed twice ties with itself: no winner to compare)


def _draw(m, kind, rng, hint=None):
    """one operation of `kind` for the model's state, or None when the state has no room for it"""
    s, M, N = m.shape, m.M, m.shape.N
    hint = hint or {}
    op = dict(kind=kind)
    off = [j for j in range(m.R) if m.windows[j] < 0]
    on = [j for j in range(m.R) if m.windows[j] >= 0]
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    fresh_k = [k for k in slide_ks(N) if k not in hint.get("used_k", ())] or slide_ks(N)   # (every k before any k twice)
    wroom = s.window_ok and m.wreads < s.wcap
    if kind == "append":
        how = pick(["one", "small", "small", "slab"] if not m.slab_done else ["one", "small"])
        how = hint.get("how", how)
        op.update(how=how, count=1 if how == "one" else int(rng.integers(8, 13)) if how == "small" else s.slab,
                  dseed=int(rng.integers(1 << 30)))
    elif kind in ("stage_commit", "refuse_slide_staged"):
        count = int(rng.integers(1, 13))
        op.update(count=count, dseed=int(rng.integers(1 << 30)))
        if kind == "stage_commit":
            cuts = sorted(set([0, count] + [int(c) for c in rng.integers(1, max(2, count), size=int(rng.integers(0, 3)))]))
            cuts = [c for c in cuts if c <= count]
            pieces = [[a, b - a] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
            op["pieces"] = [pieces[i] for i in rng.permutation(len(pieces))]
        else:
            op["k"] = int(pick(slide_ks(N)))
    elif kind == "append_from":
        op["idx"] = _idx(rng, SRC_ROWS, 1, 12, distinct=False)
    elif kind == "slide":
        if M < 1:
            return None
        whole = rng.random() < 0.5 and s.cls != "f" and not hint.get("sub")
        first = 0 if whole else int(rng.integers(1 if M > 1 else 0, M))   # (a sub-range: `first` > 0)
        count = M if whole else int(rng.integers(1, M - first + 1))
        op.update(first=first, count=count, k=int(pick(fresh_k)), dseed=int(rng.integers(1 << 30)))
    elif kind in ("slide_score", "slide_run"):
        if not wroom or M < 1:
            return None
        cand = hint.get("packed") or list(range(m.R))
        j = pick(cand)
        L = m.windows[j] if m.windows[j] >= 0 else int(pick([0, 7, 15, 16, 63]))
        op.update(j=j, k=int(pick(fresh_k)), L=L, dseed=int(rng.integers(1 << 30)))
        if kind == "slide_run":
            op.update(_run_params(m, rng))
            op["max_lag"] = L
    elif kind in ("drop_cache", "trim"):
        pass
    elif kind == "window":
        if not s.window_setting:
            return None
        j = int(rng.integers(m.R))
        op.update(j=j, L=int(pick([L for L in WINDOWS if L != m.windows[j]])))
    elif kind in ("screening", "cache_limits", "reuse"):
        cur = dict(screening=m.screening, cache_limits=m.cache_limits, reuse=m.reuse)[kind]
        op["on"] = (not cur) if rng.random() < 0.8 else cur
        if "on" in hint:
            op["on"] = bool(hint["on"])
        if kind == "screening" and op["on"] and s.screen_ok and not off:
            return None                                                # (the screened Run that follows needs a batch without a window)
    elif kind in ("scores", "run", "run_groups"):
        cand = [j for j in range(m.R) if m.windows[j] < 0 or wroom]
        if hint.get("screened"):
            cand = off
        if not cand or M < 1:
            return None
        op["j"] = hint["j"] if hint.get("j") in cand else pick(cand)
        if kind != "scores":
            op.update(_run_params(m, rng, screened=bool(hint.get("screened"))))
            if kind == "run_groups" and op["G"] == 0:
                op["G"] = int(rng.integers(1, max(2, M)))
    elif kind in ("scores_many", "run_many"):
        if not off:
            return None
        op["js"] = [off[i] for i in rng.permutation(len(off))][:int(rng.integers(1, len(off) + 1))]
        if len(off) >= 2 and len(op["js"]) < 2 and rng.random() < 0.7:
            op["js"] = [off[i] for i in rng.permutation(len(off))]
        if kind == "run_many":
            op.update(_run_params(m, rng))
    elif kind in ("scores_many_w", "run_many_w"):
        if not wroom:
            return None
        L = m.windows[pick(on)] if on and rng.random() < 0.5 else int(pick([0, 7, 15, 16, 63]))
        js = [j for j in range(m.R) if m.windows[j] in (-1, L)]
        if not js:
            return None
        op.update(js=[js[i] for i in rng.permutation(len(js))], L=L)
        if kind == "run_many_w":
            op.update(_run_params(m, rng))
            op["max_lag"] = L
    elif kind == "run_group_rows":
        src = "src" if rng.random() < 0.15 else "dg"
        op.update(src=src, idx=_idx(rng, SRC_ROWS if src == "src" else M), abs=bool(rng.random() < 0.5))
    elif kind in ("run_rows", "run_rows_w"):
        if kind == "run_rows_w" and not wroom:
            return None
        op.update(idx=_idx(rng, M), abs=bool(rng.random() < 0.5))
        if kind == "run_rows_w":
            op["L"] = int(pick([0, 7, 15, 16, 63]))
    elif kind == "muse_run":
        op["idx"] = _idx(rng, s.M0)
    elif kind == "read":
        first = int(rng.integers(0, M))
        op.update(first=first, count=int(rng.integers(1, M - first + 1)))
    elif kind == "refuse_window_f32":
        op.update(j=int(rng.integers(m.R)), L=int(pick([0, 7, 15, 16, 63])))
    elif kind == "refuse_windowed_template":
        if not on:
            return None
        op["j"] = pick(on)
    elif kind == "refuse_slide_score_window":
        if not on:
            return None
        j = pick(on)
        op.update(j=j, L=int(pick([L for L in (0, 7, 15, 16, 63) if L != m.windows[j]])), k=int(pick(slide_ks(N))),
                  dseed=int(rng.integers(1 << 30)))
    elif kind == "refuse_slide_k":
        pass
    else:
        raise KeyError(kind)
    return op if m.precondition(op) else None


def pairs_of(ops):
    """the ordered pairs (mutator or setting family -> reader family) with no other mutator between the two"""
    out, mut, sets = set(), None, []
    for op in ops:
        g, fam = GROUP[op["kind"]], FAMILY.get(op["kind"])
        if g == "mutator" or op["kind"] == "refuse_slide_staged":      # (the staged refusal commits its rows: a mutator too)
            mut, sets = (fam if g == "mutator" else None), []
        elif g == "setting":
            sets.append(fam)
        elif g == "reader":
            if op["kind"] in ("run_rows", "run_rows_w", "muse_run") or op.get("src") == "src":
                continue                                               # (rows from the host or from the other group: the reader never meets this group's state)
            if mut:
                out.add((mut, fam))
            for f in sets:
                out.add((f, fam))
    return out


def applicable_families(cls):
    """(mutator families, setting families) the class has room for at all"""
    s = Shape(cls)
    muts = ["append", "append_from", "slide", "trim"] + (["stage_commit"] if s.stage_ok else []) + \
           (["slide_score"] if s.window_ok else []) + (["drop_cache"] if s.cache else [])
    sets = ["screening", "reuse"] + (["window"] if s.window_setting else []) + (["cache_limits"] if s.cache else [])
    return muts, sets


def generate(cls, seed):
    """the operation list of (class, seed).  Stretches of one mutator, a few settings and a few readers, every draw weighted towards
    the (mutator or setting -> reader) pairs the sequence has not held yet; a refusal now and then, each followed by a reader"""
    s = Shape(cls)
    m = Model(cls, seed)
    rng = np.random.default_rng([int(seed), ord(cls), 0x6E])
    muts, sets = applicable_families(cls)
    want = {(a, r) for a in muts + sets for r in READER_FAMILIES}
    ops = []

    def emit(kind, hint=None):
        if len(ops) >= s.steps:
            return None
        op = _draw(m, kind, rng, dict(hint or {}, used_k={o["k"] for o in ops if "k" in o}))
        if op is None:
            return None
        assert m.precondition(op), op
        m.apply(op, m.prepare(op))
        ops.append(op)
        return op

    def choose(kinds, gain):
        wts = np.array([WEIGHT.get(k, 1) * (1.0 + 20.0 * gain(k)) for k in kinds], dtype=float)
        return kinds[int(rng.choice(len(kinds), p=wts / wts.sum()))]

    packed_hint = None
    if s.scale30:
        # the class exists for the dense hand-off list and its learning across a slide: two passes of one batch over the first rows
        # (the second one has learned), a slide, and two passes again; everything around them is drawn like every other class's
        emit("scores", dict(j=0))
        emit("run", dict(j=0))
        emit("slide" if rng.random() < 0.5 else "slide_score")
        emit("scores", dict(j=0))
        emit("run", dict(j=0))
        emit("run_groups", dict(j=0))
    elif s.cache:
        # the class exists for the spectrum cache: the limits lowered, two passes (the second builds), a slide under the built cache
        # and the pass behind it, the cache rebuilt, an append (one more segment) and two passes, a drop and the pass behind it
        emit("cache_limits", dict(on=True))
        emit("scores", dict(j=0))
        emit("run", dict(j=0))
        emit("slide" if rng.random() < 0.5 else "slide_score", dict(sub=True))
        emit("scores", dict(j=0))
        emit("run_groups", dict(j=0))
        emit("append", dict(how="small"))
        emit("scores", dict(j=0))
        emit("run", dict(j=0))
        emit("drop_cache")
        emit("scores", dict(j=0))
    while len(ops) < s.steps:
        missing = want - pairs_of(ops)
        # the mutator of the stretch
        mk = choose(MUTATORS, lambda k: sum(1 for p in missing if p[0] == FAMILY[k]))
        if packed_hint and s.window_ok and rng.random() < 0.6:
            mk = "slide_score"
        mop = emit(mk, dict(packed=packed_hint) if packed_hint else None)
        packed_hint = None
        if mop is None:
            continue
        stretch = [FAMILY[mk]]
        for _ in range(int(rng.integers(0, 3))):
            sk = choose(SETTINGS, lambda k: sum(1 for p in missing if p[0] == FAMILY[k]))
            sop = emit(sk)
            if sop is not None:
                stretch.append(FAMILY[sk])
                if sk == "screening" and sop["on"] and s.screen_ok:
                    emit("run", dict(screened=True))                   # at least one Run of the sequence takes the screened path
        for r in range(6):
            missing = want - pairs_of(ops)
            gain = lambda k: 0 if k in ("run_rows", "run_rows_w", "muse_run") else sum(1 for a in stretch if (a, FAMILY[k]) in missing)
            if r >= 2 and not any(gain(k) for k in READERS) and rng.random() < 0.7:
                break
            rop = emit(choose(READERS, gain))
            if rop is not None and rop["kind"] in ("scores_many_w", "run_many_w") and len(rop["js"]) >= 2 and rop["L"] <= 16 and \
                    rng.random() < 0.5:
                packed_hint = list(rop["js"])
                break                                                  # (the next stretch slides one of them: the packed origin goes stale there)
        if rng.random() < 0.2:
            fk = REFUSALS[int(rng.integers(len(REFUSALS)))]
            if emit(fk) is not None:
                for _ in range(8):
                    if emit(READERS[int(rng.integers(len(READERS)))]) is not None:
                        break
    return ops


def walk(cls, seed, ops=None):
    """(model, op, data) in front of every operation of the sequence -- the model is the live one: copy what must be kept"""
    m = Model(cls, seed)
    for op in (generate(cls, seed) if ops is None else ops):
        ok = m.precondition(op)
        d = m.prepare(op)
        yield m, op, d, ok
        m.apply(op, d)


# ------------------------------------------------------------------ expectations
def windowed_block(cc, valid, n, L):
    """_window.windowed_fast over the rows of a block of correlations at once: (lag, mv, tie); ~valid: the oracle's (nil, 0, 0)"""
    idx = W.window_indices(n, L)
    m = cc.shape[0]
    ar = np.arange(m)
    with np.errstate(all="ignore"):
        a = np.abs(cc[:, idx])
        a = np.where(np.isnan(a), -1.0, a)
        k = np.argmax(a, axis=1)                                       # the first maximum = strict '>' in scan order
        mi = np.where(a[ar, k] > 0, idx[k], 0)
        mv = cc[ar, mi]
        u = np.abs(cc[:, np.unique(idx)])
        u = np.where(np.isfinite(u), u, -np.inf)
        tie = np.zeros(m, dtype=bool)
        if u.shape[1] >= 2:
            top = np.partition(u, u.shape[1] - 2, axis=1)[:, -2:]
            tie = (top[:, 1] > 0) & ((top[:, 1] - top[:, 0]) <= W.TIE_GAP * top[:, 1])
    lag = np.where(mi <= n // 2, mi, mi - n).astype(np.int32)
    return np.where(valid, lag, 0).astype(np.int32), np.where(valid, mv, 0.0), tie & valid


class Expect:
    """oracle results per (reference, row contents): a row that an operation did not touch costs nothing the second time"""
    LS = tuple(L for L in WINDOWS if L >= 0)

    def __init__(self, oracle, refs, n):
        self.oracle, self.refs, self.n = oracle, refs, n
        self.X = [None] * len(refs)
        self.g = [dict() for _ in refs]
        self.w = [dict() for _ in refs]
        self._last = (None, None)

    def _keys(self, rows):
        if rows is self._last[0]:                                      # (the model makes a new array whenever its rows change)
            return self._last[1]
        rows = np.ascontiguousarray(rows)
        keys = [hashlib.blake2b(rows[r].tobytes(), digest_size=16).digest() for r in range(rows.shape[0])]
        self._last = (rows, keys)
        return keys

    def scores(self, j, rows):
        """(lag, mv, gap) of oracle.batch_scores for reference j"""
        keys = self._keys(rows)
        c = self.g[j]
        miss = [i for i, k in enumerate(keys) if k not in c]
        if miss:
            lag, mv, gap = self.oracle.batch_scores(self.refs[j], np.ascontiguousarray(rows[miss]), nthreads=8)
            for t, i in enumerate(miss):
                c[keys[i]] = (int(lag[t]), float(mv[t]), float(gap[t]))
        out = [c[k] for k in keys]
        return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out]), np.array([o[2] for o in out]))

    def windowed(self, j, rows, L):
        """(lag, mv, tie) by the lag window's definition (_window.py) for reference j"""
        keys = self._keys(rows)
        c = self.w[j]
        miss = [i for i, k in enumerate(keys) if k not in c]
        if miss:
            if self.X[j] is None:
                self.X[j] = self.oracle.ref_spectrum(self.refs[j])[0]
            for lo in range(0, len(miss), 256):
                part = miss[lo:lo + 256]
                cc = np.zeros((len(part), self.n))
                valid = np.ones(len(part), dtype=bool)
                for t, i in enumerate(part):
                    one = self.oracle.xcorr_with_x(self.X[j], rows[i], self.n)[0]
                    if one is None:
                        valid[t] = False
                    else:
                        cc[t] = one
                per = {Lw: windowed_block(cc, valid, self.n, Lw) for Lw in self.LS}
                for t, i in enumerate(part):
                    c[keys[i]] = {Lw: (int(per[Lw][0][t]), float(per[Lw][1][t]), bool(per[Lw][2][t])) for Lw in self.LS}
        out = [c[k][L] for k in keys]
        return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out]), np.array([o[2] for o in out], dtype=bool))

    def forget(self, rows):
        """keep only what describes these rows (memory)"""
        live = set(self._keys(rows))
        for c in self.g + self.w:
            for k in [k for k in c if k not in live]:
                del c[k]


# ------------------------------------------------------------------ the runner
class Runner:
    def __init__(self, muse, eng, oracle, cls, seed, ops=None):
        self.muse, self.eng, self.oracle, self.cls, self.seed = muse, eng, oracle, cls, int(seed)
        self.ops = generate(cls, seed) if ops is None else list(ops)
        self.m = Model(cls, seed)
        self.exp = Expect(oracle, self.m.refs, self.m.shape.n)
        self.bits = {}           # (batch, rows version, window or kernel) -> the bytes of an all-scores pass
        self.all = {}            # (batch, rows version, window) -> (lag, mv) of an all-scores pass that has been held to the oracle
        self.pending_rows = False
        self.screen_switched_on = False
        self.screened_runs = 0
        self.kernels = set()     # every kernel name a batch reported
        self.cache_seen = False  # the group held a valid spectrum cache at some step
        self.learned = {}        # batch -> the rows version its last fp64 all-scores pass of its own saw (class g: the learned hand-off)
        self.handles = []

    # ---- set-up and tear-down
    def _open(self):
        muse, eng, m, s = self.muse, self.eng, self.m, self.m.shape
        self.B = muse.binding
        from test_gpu_lag_window import check
        from test_gpu_parity import assert_scores_match
        from test_gpu_window_rows import assert_winner, winner
        self.check, self.assert_scores_match, self.assert_winner, self.winner = check, assert_scores_match, assert_winner, winner
        self.dg = muse.DeviceGroup(eng, s.N, s.M0, f32=s.f32)
        self.dg.append(m.initial_raw)      # (unrounded: a float32 group narrows them itself)
        self.src = muse.DeviceGroup.from_rows(eng, m.src_rows, f32=s.f32)
        self.dbs = [muse.DeviceBatch(eng, self.dg, ref) for ref in m.refs]
        self.tgroup = muse.DeviceGroup(eng, s.N, 0)
        self.tmpl = muse.DeviceBatch.like(self.dbs[0], self.tgroup)
        self.handles = self.dbs + [self.tmpl, self.tgroup, self.src, self.dg]
        # the mirror's Muse.Run over Series whose home is the group: what they hold is what the rows were when they were added
        self.series = [muse.NewSeries(m.rows[r].copy(), muse.NewLabels({"i": str(r)})) for r in range(s.M0)]
        for r, sr in enumerate(self.series):
            muse.muse.set_home(sr, self.dg, r)
        self.results = muse.NewResults(s.N, 1, 0.0, muse.SignFilter_ANY)
        self.mirror = muse.New(muse.NewSeries(m.refs[0]), self.results, engine=eng)
        self.check_rows()

    def _close(self):
        eng = self.eng
        eng.set_screening(False)
        eng.spectrum_cache_limits()
        eng.reuse_resident_rows(True)
        mirror = getattr(self, "mirror", None)
        err = None
        for h in ([mirror._template, mirror._probe] if mirror is not None else []) + self.handles:
            try:
                h.close()
            except Exception as e:     # (the others are still closed; the first failure is reported)
                err = err or e
        if err is not None:
            raise err

    def run(self):
        s = self.m.shape
        i = -1
        try:
            self._open()
            for i, op in enumerate(self.ops):
                self.step(op)
            self.check_rows()
            if self.screen_switched_on and s.screen_ok:
                assert self.screened_runs >= 1, "screening was switched on and no Run reported MUSE_RUN_PATH_SCREENED"
        except BaseException:
            print("\nSEQUENCE FAILED: class %s seed %d step %d of %d: %s" % (self.cls, self.seed, i, len(self.ops),
                                                                             json.dumps(self.ops[i]) if 0 <= i < len(self.ops) else "set-up"))
            print("replay: _seq.replay(muse, eng, oracle, %r, %d, json.loads(%r))" % (self.cls, self.seed, json.dumps(self.ops[:i + 1])))
            raise
        finally:
            self._close()

    # ---- checks shared by the steps
    def check_rows(self):
        m = self.m
        self.pending_rows = False
        assert self.dg.M == m.M, (self.dg.M, m.M)
        got = self.dg.read(0, m.M) if m.M else np.zeros((0, m.shape.N))
        if got.tobytes() != m.rows.tobytes():
            bad = np.argwhere(got.view(np.uint64) != m.rows.view(np.uint64))
            raise AssertionError("rows differ from the model at (row, sample) %s ..." % bad[:4].tolist())

    def check_state(self):
        """what no operation may leave wrong: the row count, the slide counter, every batch's window and the kernel its scores name"""
        m, n = self.m, self.m.shape.n
        assert self.dg.M == m.M and self.dg.slides == m.slides, (self.dg.M, m.M, self.dg.slides, m.slides)
        for j, db in enumerate(self.dbs):
            assert db.lag_window() == m.windows[j], (j, db.lag_window(), m.windows[j])
            name = self.eng.kernel_name(db)
            self.kernels.add(name)
            if m.packed[j]:
                assert name.startswith("xcorr_window_many_mfma<"), (j, name)
            elif m.windows[j] >= 0:
                tiles = (2 * min(m.windows[j], n // 2) + 1 + 15) // 16
                assert name.startswith("xcorr_window_mfma<%d," % tiles), (j, name, m.windows[j])
            else:
                assert not name.startswith("xcorr_window"), (j, name)
                if m.shape.scale30:
                    # mixed units: a pass over these rows lists every pair, and the next one goes to the rescaling kernel directly -- but
                    # only over the rows that pass saw: behind a slide or an append the batch is back on the default kernel and relearns
                    assert (name == "xcorr_fused_n4096_occ4") == (self.learned.get(j) == m.version), (j, name, self.learned.get(j), m.version)
        assert self.tmpl.lag_window() == -1
        self.cache_seen = self.cache_seen or self.dg.spectrum_cache()[0] > 0

    def _stable(self, j, what, lag, mv):
        """bit stability: while the rows, the batch's window and the selected kernel are the same, two all-scores passes agree bit for bit"""
        key = (j, self.m.version, what)
        blob = lag.tobytes() + mv.tobytes()
        if key in self.bits:
            if self.bits[key] != blob:
                old = np.frombuffer(self.bits[key][lag.nbytes:], dtype=np.float64)
                raise AssertionError("two passes of batch %d over the same rows (%s) differ in bits at rows %s"
                                     % (j, what, np.flatnonzero(old.view(np.uint64) != mv.view(np.uint64))[:8]))
        else:
            for k in [k for k in self.bits if k[1] != self.m.version]:
                del self.bits[k]
            self.bits[key] = blob

    def held(self, j, lag, mv, L, stable=None):
        """an all-scores result of batch j at window L (-1: none) against the oracle on the model's rows"""
        m = self.m
        assert len(lag) == m.M == len(mv)
        keep = m.keep()
        if L < 0:
            olag, omv, gap = self.exp.scores(j, m.rows)
            self.assert_scores_match(lag, mv, olag, omv, gap, max_ties=m.M // 1000)
            tie = (gap < W.TIE_GAP) & ~np.isnan(omv) & keep
            assert int(tie.sum()) * 1000 <= int(keep.sum()), "%d tied rows of %d" % (int(tie.sum()), int(keep.sum()))
        else:
            elag, emv, tie = self.exp.windowed(j, m.rows, min(L, m.shape.n // 2))
            self.check(lag, mv, elag, emv, tie, keep, cap_ties=True)
            assert np.all(np.abs(lag) <= L)
        if stable is not None:
            self._stable(j, stable, lag, mv)

    def _kernel(self, j):
        name = self.eng.kernel_name(self.dbs[j])
        # (the spectrum cache's reader is documented bit-identical to the kernel it replaces: DESIGN 4.10)
        return "n4096 fold / cached" if name.startswith(("xcorr_cached_n4096", "xcorr_fused_n4096_fold")) else name

    def all_scores(self, j):
        """(lag, mv) of batch j's all-scores pass for the state as it is, held to the oracle (a new pass unless one is known)"""
        m = self.m
        key = (j, m.version, m.windows[j])
        if key not in self.all:
            lag, mv = self.dbs[j].scores()
            m.packed[j] = False
            self.learned[j] = m.version
            L = m.windows[j]
            self.held(j, lag, mv, L, stable=("w", L) if L >= 0 else ("k", self._kernel(j)))
            for k in [k for k in self.all if k[1] != m.version]:
                del self.all[k]
            self.all[key] = (lag, mv)
        return self.all[key]

    def _same_run(self, got, lag, mv, op, gid, rtol=0.0):
        exp = self.oracle.results(lag, mv, gid, op["G"], op["abs"], op["max_lag"], op["top_n"], op["thr"], op["sign"])
        assert got[0].tolist() == exp[0].tolist(), (got[0][:8], exp[0][:8])
        assert got[1].tolist() == exp[1].tolist()
        if rtol:
            np.testing.assert_allclose(got[2], exp[2], rtol=rtol, atol=0)
            assert (math.isnan(got[3]) and math.isnan(exp[3])) or abs(got[3] - exp[3]) <= rtol * max(1.0, abs(exp[3]))
        else:
            assert np.array_equal(got[2], exp[2], equal_nan=True)
            assert (math.isnan(got[3]) and math.isnan(exp[3])) or abs(got[3] - exp[3]) <= 1e-15 * max(1.0, abs(exp[3]))

    def _screen_rtol(self):
        # a screened Run's scores come from the re-evaluating kernel: test_gpu_parity.py (the screened Run against the all-scores pass)
        N = self.m.shape.N
        return 5e-11 if (2048 < N < 4096 or N > 4096) else 1e-12

    def _refused(self, fn, status):
        try:
            fn()
        except self.B.MuseError as e:
            assert e.status == status, (e.status, status, str(e))
            return
        raise AssertionError("the call was not refused")

    # ---- one step
    def step(self, op):
        m, kind = self.m, op["kind"]
        assert m.precondition(op), op
        if self.pending_rows and (GROUP[kind] in ("mutator", "refusal")):
            self.check_rows()
        d = m.prepare(op)
        getattr(self, "do_" + kind)(op, d)
        if GROUP[kind] == "mutator":
            # (every other time the rows are read back only behind the next reader: the reader then meets the uploads still in flight)
            if op.get("dseed", 0) % 2 == 0:
                self.check_rows()
            else:
                self.pending_rows = True
        elif GROUP[kind] == "reader" and self.pending_rows:
            self.check_rows()
        if GROUP[kind] == "refusal":
            self.check_rows()
        self.check_state()

    # ---- mutators
    def do_append(self, op, d):
        if op["how"] == "one":
            self.dg.append(d["rows"][0])
        else:
            self.dg.append(d["rows"])
        self.m.apply(op, d)

    def do_stage_commit(self, op, d):
        win = self.dg.stage(op["count"])
        assert win.shape[0] == op["count"]
        win[:, :] = d["rows"]
        for first, count in op["pieces"]:
            self.dg.commit(first, count)
        self.m.apply(op, d)

    def do_append_from(self, op, d):
        self.dg.append_from(self.src, op["idx"])
        self.m.apply(op, d)

    def do_slide(self, op, d):
        self.dg.slide(d["tails"], first=op["first"])
        self.m.apply(op, d)

    def do_slide_score(self, op, d):
        j = op["j"]
        self.dbs[j].slide_score_windowed(d["tails"], op["L"])
        self.m.apply(op, d)
        lag, mv = self.dbs[j].read_scores()
        self.held(j, lag, mv, op["L"], stable=("w", op["L"]))

    def do_slide_run(self, op, d):
        j, db = op["j"], self.dbs[op["j"]]
        got = db.slide_run_windowed(d["tails"], op["L"], d["gid"], op["G"], op["top_n"], op["thr"], op["sign"], op["abs"])
        assert db.last_run_path() == 0
        self.m.apply(op, d)
        lag, mv = db.read_scores()
        self.held(j, lag, mv, op["L"], stable=("w", op["L"]))
        self._same_run(got, lag, mv, op, d["gid"])

    def do_drop_cache(self, op, d):
        self.dg.drop_spectrum_cache()
        assert self.dg.spectrum_cache() == (0, 0)
        self.m.apply(op, d)

    def do_trim(self, op, d):
        self.eng.trim()
        self.m.apply(op, d)

    # ---- settings
    def do_window(self, op, d):
        self.dbs[op["j"]].set_lag_window(op["L"])
        self.m.apply(op, d)

    def do_screening(self, op, d):
        self.eng.set_screening(op["on"], min_rows=2)
        self.screen_switched_on = self.screen_switched_on or op["on"]
        self.m.apply(op, d)

    def do_cache_limits(self, op, d):
        if op["on"]:
            self.eng.spectrum_cache_limits(min_rows=64)
        else:
            self.eng.spectrum_cache_limits()
        self.m.apply(op, d)

    def do_reuse(self, op, d):
        self.eng.reuse_resident_rows(op["on"])
        self.m.apply(op, d)

    # ---- readers
    def do_scores(self, op, d):
        j, m = op["j"], self.m
        lag, mv = self.dbs[j].scores()
        self.learned[j] = m.version
        m.apply(op, d)
        L = m.windows[j]
        self.held(j, lag, mv, L, stable=("w", L) if L >= 0 else ("k", self._kernel(j)))
        self.all[(j, m.version, L)] = (lag, mv)

    def do_run(self, op, d):
        j, m, db = op["j"], self.m, self.dbs[op["j"]]
        got = db.run(d["gid"], op["G"], op["max_lag"], op["top_n"], op["thr"], op["sign"], op["abs"])
        path = db.last_run_path()
        m.apply(op, d)
        if path != 1:
            self.learned[j] = m.version
        if m.screen_eligible(op):
            assert path in (1, 2, 3), path
        else:
            assert path == 0, path
        self.screened_runs += path == 1
        lag, mv = self.all_scores(j)
        # a screened Run must select exactly what the fp64 Run selects (its scores: the re-evaluating kernel's)
        self._same_run(got, lag, mv, op, d["gid"], rtol=self._screen_rtol() if path == 1 else 0.0)

    def do_run_groups(self, op, d):
        j, m, db = op["j"], self.m, self.dbs[op["j"]]
        rec, state = db.run_groups(d["gid"], op["G"], 0, abs_scores=op["abs"])
        self.learned[j] = m.version
        m.apply(op, d)
        wrec, wstate = self.muse.merge_group_winners(rec[None, :], state[None, :])
        got = self.muse.merge_group_records(wrec[None, :], wstate[None, :], op["max_lag"], op["top_n"], op["thr"], op["sign"])
        lag, mv = self.all_scores(j)
        self._same_run(got, lag, mv, op, d["gid"])

    def do_scores_many(self, op, d):
        got = self.muse.scores_many([self.dbs[j] for j in op["js"]])
        self.m.apply(op, d)
        if len(op["js"]) == 1:         # (one reference: the batch's own pass; several: the one-pass kernel, which learns nothing)
            self.learned[op["js"][0]] = self.m.version
        for j, (lag, mv) in zip(op["js"], got):
            self.held(j, lag, mv, -1)

    def do_run_many(self, op, d):
        dbs = [self.dbs[j] for j in op["js"]]
        got = self.muse.run_many(dbs, d["gid"], op["G"], op["max_lag"], op["top_n"], op["thr"], op["sign"], op["abs"])
        self.m.apply(op, d)
        for j, db, res in zip(op["js"], dbs, got):
            path = db.last_run_path()
            self.screened_runs += path == 1
            lag, mv = db.read_scores()           # the pass's own results (a screened one: re-scored in fp64 here)
            if path == 1 or len(dbs) == 1:
                self.learned[j] = self.m.version
            self.held(j, lag, mv, -1)
            self._same_run(res, lag, mv, op, d["gid"], rtol=self._screen_rtol() if path == 1 else 0.0)

    def _packed_of(self, op):
        R, L = len(op["js"]), min(op["L"], self.m.shape.n // 2)
        plan = self.muse.window_many_plan(R, L)
        of = plan["launch_of"].tolist()
        return [of.count(of[r]) > 1 for r in range(R)]

    def do_scores_many_w(self, op, d):
        got = self.muse.scores_many_windowed([self.dbs[j] for j in op["js"]], op["L"])
        self.m.apply(op, d)
        for j, p, (lag, mv) in zip(op["js"], self._packed_of(op), got):
            self.m.packed[j] = p
            self.held(j, lag, mv, op["L"], stable=("w", op["L"]))

    def do_run_many_w(self, op, d):
        dbs = [self.dbs[j] for j in op["js"]]
        got = self.muse.run_many_windowed(dbs, d["gid"], op["G"], op["L"], op["top_n"], op["thr"], op["sign"], op["abs"])
        self.m.apply(op, d)
        for j, p, db, res in zip(op["js"], self._packed_of(op), dbs, got):
            self.m.packed[j] = p
            assert db.last_run_path() == 0
            lag, mv = db.read_scores()
            self.held(j, lag, mv, op["L"], stable=("w", op["L"]))
            self._same_run(res, lag, mv, op, d["gid"])

    def _winner_of(self, rows, abs_scores, L=-1):
        if L < 0:
            lag, mv, _ = self.exp.scores(0, rows)
        else:
            lag, mv, _ = self.exp.windowed(0, rows, L)
        return self.winner(lag, mv, abs_scores)

    def do_run_group_rows(self, op, d):
        src, rows = (self.src, self.m.src_rows) if op["src"] == "src" else (self.dg, self.m.rows)
        idx = np.array(op["idx"], dtype=np.int64)
        got = self.tmpl.run_group_rows(src, idx, op["abs"])
        self.m.apply(op, d)
        self.assert_winner(got, self._winner_of(rows[idx], op["abs"]))

    def do_run_rows(self, op, d):
        rows = self.m.rows[np.array(op["idx"], dtype=np.int64)]
        got = self.tmpl.run_rows(rows, op["abs"])
        self.m.apply(op, d)
        self.assert_winner(got, self._winner_of(rows, op["abs"]))

    def do_run_rows_w(self, op, d):
        rows = self.m.rows[np.array(op["idx"], dtype=np.int64)]
        got = self.tmpl.run_rows_windowed(rows, op["L"], op["abs"])
        self.m.apply(op, d)
        self.assert_winner(got, self._winner_of(rows, op["abs"], op["L"]))

    def do_muse_run(self, op, d):
        """the mirror's Muse.Run over Series added before the first slide: from the group's rows while their home is alive and reuse is
        on, from the host once the group has slid -- either way what the Series hold"""
        m = self.m
        ser = [self.series[i] for i in op["idx"]]
        home = self.mirror._resident(ser)
        assert (home is not None) == (m.reuse and m.slides == 0), (home is not None, m.reuse, m.slides)
        self.mirror.Run(ser)
        got, _ = self.results.Fetch()
        m.apply(op, d)
        k, lag, score, state, gap = self._winner_of(np.stack([sr.y for sr in ser]), False)
        if state == 1 and k >= 0:
            assert gap > 1e-7 and len(got) == 1
            assert got[0].Labels.labels["i"] == str(op["idx"][k]) and got[0].Lag == lag
            assert abs(got[0].PercentScore - score) <= 1e-6 * abs(score) + 1e-12
        else:
            assert got == []

    def do_read(self, op, d):
        got = self.dg.read(op["first"], op["count"])
        self.m.apply(op, d)
        assert got.tobytes() == self.m.rows[op["first"]:op["first"] + op["count"]].tobytes()

    # ---- refusals that must change nothing (step() then reads the rows back and checks every window and the slide counter)
    def do_refuse_window_f32(self, op, d):
        self._refused(lambda: self.dbs[op["j"]].set_lag_window(op["L"]), self.B.MUSE_ERR_UNSUPPORTED)
        self.m.apply(op, d)

    def do_refuse_windowed_template(self, op, d):
        rows = self.m.rows[:min(4, self.m.M)]
        self._refused(lambda: self.dbs[op["j"]].run_rows(rows), self.B.MUSE_ERR_UNSUPPORTED)
        self.m.apply(op, d)

    def do_refuse_slide_score_window(self, op, d):
        self._refused(lambda: self.dbs[op["j"]].slide_score_windowed(d["tails"], op["L"]), self.B.MUSE_ERR_INVALID)
        self.m.apply(op, d)

    def do_refuse_slide_staged(self, op, d):
        """an open staging window refuses the slide; the window is then filled and committed (nothing else closes it)"""
        m = self.m
        win = self.dg.stage(op["count"])
        assert win.shape[0] == op["count"]
        self._refused(lambda: self.dg.slide(np.zeros((m.M, op["k"]))), self.B.MUSE_ERR_INVALID)
        assert self.dg.slides == m.slides
        win[:, :] = d["rows"]
        self.dg.commit(0, op["count"])
        m.apply(op, d)

    def do_refuse_slide_k(self, op, d):
        self._refused(lambda: self.dg.slide(np.zeros((self.m.M, self.m.shape.N + 1))), self.B.MUSE_ERR_INVALID)
        self.m.apply(op, d)


def replay(muse, eng, oracle, cls, seed, ops=None):
    """run the sequence of (class, seed) -- or the given operation list over that seed's initial state -- on the device"""
    Runner(muse, eng, oracle, cls, seed, ops).run()
