"""What go-muse_amd/muse.py asks of the C library and of Results, recorded without a device or a built library.

Level 1: binding.load is replaced by a stand-in whose every muse_* attribute logs its call -- the name, scalar arguments by
value (converted as the entry point's argtypes in binding.SIGNATURES would convert them), pointer arguments by ctypes type and
NULL-ness (and by the name of the driver's input array they point into) -- fills the outputs with fixed values and returns
MUSE_OK.  A DeviceBatch made with object.__new__ is driven through every call-shape method, and the plan functions with it.
Level 2: Batch and Muse objects get a device side that logs the DeviceBatch method and its arguments (bound to the real method's
signature, so positional and keyword spellings log alike) and returns canned results; the log also holds every Results.Update
and the status and message of every MuseError.
Signatures: inspect.signature and a digest of the docstring of every public callable of muse.py and of the public methods of
DeviceBatch, Batch and Muse.

record() returns all of it; tests/golden/python_mirror_calls.json is the committed record and
tests/test_python_mirror_cpu.py compares the two line by line.  `python tests/_mirrorlog.py --write` regenerates the file:
only a change that MEANS to alter a call, a feed or a signature does that.
"""
import contextlib
import ctypes
import hashlib
import inspect
import json
import operator
import os
import sys
import weakref

import numpy as np

from _load import ROOT, pkg

FIXTURE = os.path.join(ROOT, "tests", "golden", "python_mirror_calls.json")

_INT_TYPES = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint8)
_SELECTION_TAIL = ("LP_c_long", "LP_c_int", "LP_c_double", "LP_c_int", "LP_c_double")   # o_s, o_l, o_v, cnt, mean


def _addr(p):
    return ctypes.cast(p, ctypes.c_void_p).value


def _num(v):
    return repr(float(v)) if isinstance(v, (float, np.floating)) else repr(int(v))


# ------------------------------------------------------------------ level 1: the C library
class RecordingLib:
    """stands in for the ctypes library: lib.muse_xyz(...) logs one line and returns MUSE_OK (or `fail_next`, once)"""

    def __init__(self, M, log):
        self._M, self._log = M, log      # M: pkg().muse
        self._names = {}                 # data address -> name of a driver's input array
        self.fail_next = None

    def name(self, array, label):
        self._names[array.ctypes.data] = label
        return array

    def __getattr__(self, fn):
        if not fn.startswith("muse_"):
            raise AttributeError(fn)
        return lambda *args: self._call(fn, args)

    def _pointer(self, a):
        if a is None:
            return "NULL"
        if type(a).__name__ == "CArgObject":                       # ctypes.byref(x)
            return "&" + type(a._obj).__name__
        if isinstance(a, ctypes.Array):                            # a pointer list / a handle list
            inner = [self._pointer(x) if isinstance(x, ctypes._Pointer) else repr(x) for x in a]
            return "%s[%s]" % (type(a)._type_.__name__, ", ".join(inner))
        if isinstance(a, ctypes.c_void_p):
            return "handle(%r)" % a.value
        if isinstance(a, ctypes._Pointer):
            if not a:
                return type(a).__name__ + ":NULL"
            label = self._names.get(_addr(a))
            return type(a).__name__ + (":" + label if label else "")
        if isinstance(a, ctypes._SimpleCData):                     # ctypes.c_uint64(seed)
            return "%s(%r)" % (type(a).__name__, a.value)
        return "?" + type(a).__name__

    def _describe(self, a, argtype):
        if argtype in _INT_TYPES and not isinstance(a, ctypes._SimpleCData):
            return repr(operator.index(a))                         # what ctypes accepts for an integer parameter
        if argtype is ctypes.c_double:
            return repr(float(a))
        return self._pointer(a)

    def _call(self, fn, args):
        B = self._M.B
        if fn == "muse_last_error":
            return b"recorded failure"
        argtypes = B.SIGNATURES[fn][1]
        if len(args) != len(argtypes):
            self._log.append("%s: %d arguments for %d parameters" % (fn, len(args), len(argtypes)))
        self._log.append("%s(%s)" % (fn, ", ".join(self._describe(a, t) for a, t in zip(args, argtypes))))
        if self.fail_next is not None:
            status, self.fail_next = self.fail_next, None
            return status
        self._fill(fn, args, [t.__name__ for t in argtypes])
        return B.MUSE_OK

    def _fill(self, fn, args, types):
        """fixed outputs, so that what a wrapper returns shows how it slices and converts them"""
        def put(a, values):
            if type(a).__name__ == "CArgObject":
                a._obj.value = values[0]
            else:
                for i, v in (values.items() if isinstance(values, dict) else enumerate(values)):
                    a[i] = v
        if fn.startswith("muse_batch_") and tuple(types[-5:]) == _SELECTION_TAIL:
            # the selection shape: (..., top_n, threshold, sign_filter, abs, o_s, o_l, o_v, &cnt, &mean)
            many = types[0] == "LP_c_void_p"                       # (batches, R, ...): R x top_n outputs, cnt[R], mean[R]
            R = args[1] if many else 1
            tn = max(int(args[-9]), 0 if many else 1)
            c = min(2, tn)
            for r in range(R):
                put(args[-5], {r * tn + i: (3 - 3 * i + r) % 4 for i in range(c)})
                put(args[-4], {r * tn + i: (-1, 2)[i] + r for i in range(c)})
                put(args[-3], {r * tn + i: (0.5, -0.25)[i] / (r + 1) for i in range(c)})
            if many:
                put(args[-2], [c] * R)
                put(args[-1], [0.375 / (r + 1) for r in range(R)])
            else:
                put(args[-2], [c])
                put(args[-1], [0.375])
        elif fn == "muse_batch_run_shard":                         # (..., rec, &cnt)
            c = min(2, max(int(args[5]), 1))
            for i in range(c):
                args[-2][i].series, args[-2][i].score, args[-2][i].lag, args[-2][i].group = 3 - 3 * i, (0.5, -0.25)[i], (-1, 2)[i], i
            put(args[-1], [c])
        elif fn == "muse_batch_run_groups":                        # (h, gid, G, offset, abs, rec[G], state[G])
            for g in range(int(args[2])):
                args[-2][g].series, args[-2][g].score, args[-2][g].lag, args[-2][g].group = g + 1, 0.5 + g / 8, -g, g
                args[-1][g] = 1
        elif fn == "muse_merge_group_winners":                     # (rec[W][G], state[W][G], W, G, out[G], ost[G]): the first shard's
            for g in range(int(args[3])):
                args[-2][g], args[-1][g] = args[0][g], args[1][g]
        elif types[-2:] == ["LP_MuseRecord", "LP_c_ubyte"]:        # the winner shape: (..., abs, rec, &state)
            args[-2][0].series, args[-2][0].score, args[-2][0].lag, args[-2][0].group = 1, 0.75, -2, 0
            put(args[-1], [1])
        elif fn.endswith("_scores") and fn.startswith("muse_test_run_rows"):   # (h, rows, M, stride, ..., lag[M], mv[M])
            for i in range(int(args[2])):
                args[-2][i], args[-1][i] = i - 1, i / 8
        elif fn.startswith("muse_test_window_many_plan"):          # (R, L, &n, of, tiles, &mx, img, kc)
            R = max(int(args[0]), 1)
            put(args[2], [min(2, R)])
            put(args[5], [5])
            for i in range(R):
                args[3][i], args[4][i], args[6][i], args[7][i] = i % 2, 10 + i, 20 + i, 30 + i
        elif fn.endswith("_plan"):                                 # every trailing &int32 is an output
            k = len(types)
            while k > 0 and types[k - 1] == "LP_c_int":
                k -= 1
            for j, a in enumerate(args[k:]):
                put(a, [3 + j])


def _show(v):
    """a wrapper's return value, as text"""
    if isinstance(v, tuple):
        return "(" + ", ".join(_show(x) for x in v) + ")"
    if isinstance(v, list):
        return "[" + ", ".join(_show(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join("%s: %s" % (k, _show(v[k])) for k in v) + "}"
    if isinstance(v, np.ndarray):
        if v.dtype.names:
            return "%s[%s]" % ("record", ", ".join(_show(x) for x in v))
        return "%s%s" % (v.dtype.name, [x.item() for x in v.reshape(-1)])
    if isinstance(v, np.void):
        return "{" + ", ".join("%s=%s" % (n, _num(v[n])) for n in v.dtype.names) + "}"
    if isinstance(v, (np.generic,)):
        return "%s(%s)" % (type(v).__name__, _num(v))
    return "%s(%r)" % (type(v).__name__, v)


class _StubGroup:
    """what a DeviceBatch reads of its DeviceGroup"""

    def __init__(self, N, M, engine=None):
        self.N, self.M, self.slides = N, M, 0
        self._h = ctypes.c_void_p(0x6000)
        self.alive, self.engine, self.f32 = True, engine, False


def _bare_batch(M, handle, dgroup):
    """a DeviceBatch without a muse_batch behind it (and so nothing to free)"""
    class Bare(M.DeviceBatch):
        def close(self):
            pass
    db = object.__new__(Bare)
    db.engine, db.n, db.dgroup, db._h = None, 16, dgroup, ctypes.c_void_p(handle)
    return db


@contextlib.contextmanager
def _patched(M, lib):
    saved = M.B.load, M.EXACT_FEED_MAX_GROUPS
    M.B.load = lambda: lib
    try:
        yield
    finally:
        M.B.load, M.EXACT_FEED_MAX_GROUPS = saved


def _attempt(M, log, label, call):
    """log the call's label, then what it did: its return value or its MuseError / ValueError"""
    log.append("> " + label)
    try:
        out = call()
    except M.MuseError as e:
        log.append("  MuseError(%d, %r)" % (e.status, e.message))
    except ValueError as e:
        log.append("  ValueError(%r)" % (str(e),))
    else:
        log.append("  -> " + _show(out))


def record_c_calls(M):
    """level 1: {section: [lines]}"""
    sections = {}
    Mrows, N = 4, 8
    rows = np.arange(Mrows * N, dtype=np.float64).reshape(Mrows, N)
    wide = np.arange(Mrows * 2 * N, dtype=np.float64).reshape(Mrows, 2 * N)[:, :N]     # a row stride of 2 N
    series = [np.arange(N, dtype=np.float64) + i for i in range(3)]
    gid = np.array([1, 0, 1, 2], dtype=np.int32)
    tails = {0: np.zeros((Mrows, 0)), 2: np.arange(Mrows * 2, dtype=np.float64).reshape(Mrows, 2)}
    idx = np.array([2, 0, 3], dtype=np.int64)

    def section(title):
        log = sections[title] = []
        lib = RecordingLib(M, log)
        for arr, label in ((rows, "rows"), (wide, "wide"), (gid, "gid"), (idx, "idx"), (tails[0], "tails0"), (tails[2], "tails2")):
            lib.name(arr, label)
        for i, s in enumerate(series):
            lib.name(s, "series%d" % i)
        return log, lib, _bare_batch(M, 0x5000, _StubGroup(N, Mrows))

    # ---- the selection shape
    log, lib, db = section("DeviceBatch selection")
    with _patched(M, lib):
        sel = dict(G=3, top_n=5, threshold=0.125, sign_filter=-1, abs_scores=False)
        for g in (None, gid):
            tag = "gid" if g is not None else "None"
            _attempt(M, log, "run(%s)" % tag, lambda: db.run(g, max_lag=7, **sel))
            _attempt(M, log, "run(%s) defaults" % tag, lambda: db.run(g))
            _attempt(M, log, "run_in_window(%s)" % tag, lambda: db.run_in_window(9, g, **sel))
            _attempt(M, log, "run_in_window(%s) defaults" % tag, lambda: db.run_in_window(9, g))
            for name in ("run_in_lag_range", "run_signed_in_lag_range", "run_in_lag_band"):
                _attempt(M, log, "%s(%s)" % (name, tag), lambda: getattr(db, name)(-3, 4, g, **sel))
                _attempt(M, log, "%s(%s) defaults" % (name, tag), lambda: getattr(db, name)(-3, 4, g))
            _attempt(M, log, "run_shard(%s)" % tag, lambda: db.run_shard(g, 3, 100, 7, 5, 0.125, 1, True))
            _attempt(M, log, "run_shard(%s) defaults" % tag, lambda: db.run_shard(g))
        _attempt(M, log, "run(gid) top_n=1", lambda: db.run(gid, 3, 7, 1, 0.0, 0, True))
        _attempt(M, log, "run(gid) top_n=0", lambda: db.run(gid, 3, 7, 0, 0.0, 0, True))
        _attempt(M, log, "run(list)", lambda: db.run([1, 0, 1, 2], 3))
        _attempt(M, log, "run_groups", lambda: db.run_groups(gid, 3, 100, abs_scores=False))
        _attempt(M, log, "run_groups defaults", lambda: db.run_groups(gid, 3))
        lib.fail_next = M.B.MUSE_ERR_UNSUPPORTED
        _attempt(M, log, "run_in_lag_band refused", lambda: db.run_in_lag_band(1, 4, gid, 3))

    # ---- the slide forms
    log, lib, db = section("DeviceBatch slide")
    with _patched(M, lib):
        for k in (0, 2):
            for g in (None, gid):
                tag = "k=%d, %s" % (k, "gid" if g is not None else "None")
                for name, lead in (("slide_run_windowed", (9,)), ("slide_run_in_window", (9,)), ("slide_run", ())):
                    rest = dict(sel, max_lag=7) if name == "slide_run" else sel
                    _attempt(M, log, "%s(%s)" % (name, tag), lambda: getattr(db, name)(tails[k], *lead, g, **rest))
                    log.append("  slides = %d" % db.dgroup.slides)
                    _attempt(M, log, "%s(%s) defaults" % (name, tag), lambda: getattr(db, name)(tails[k], *lead, g))
                    log.append("  slides = %d" % db.dgroup.slides)
            for name in ("slide_score_windowed", "slide_score_in_window"):
                _attempt(M, log, "%s(k=%d)" % (name, k), lambda: getattr(db, name)(tails[k], 9))
                log.append("  slides = %d" % db.dgroup.slides)
        for name, lead in (("slide_run_windowed", (9,)), ("slide_run_in_window", (9,)), ("slide_run", ()),
                           ("slide_score_windowed", (9,)), ("slide_score_in_window", (9,))):
            lib.fail_next = M.B.MUSE_ERR_INVALID
            _attempt(M, log, "%s refused" % name, lambda: getattr(db, name)(tails[2], *lead))
            log.append("  slides = %d" % db.dgroup.slides)
            _attempt(M, log, "%s, 3 rows of tails" % name, lambda: getattr(db, name)(tails[2][:3], *lead))
            _attempt(M, log, "%s, 1-D tails" % name, lambda: getattr(db, name)(tails[2][0], *lead))
            log.append("  slides = %d" % db.dgroup.slides)
        strided = lib.name(np.arange(Mrows * 6, dtype=np.float64).reshape(Mrows, 6)[:, :2], "strided")
        _attempt(M, log, "slide_run(row stride 6)", lambda: db.slide_run(strided, gid, 3))
        _attempt(M, log, "slide_run(column stride 2: copied)", lambda: db.slide_run(strided[:, ::2], gid, 3))

    # ---- the winner shape and the per-row scores
    log, lib, db = section("DeviceBatch winner")
    with _patched(M, lib):
        src = _StubGroup(N, 10)
        forms = (("", ()), ("_windowed", (9,)), ("_in_lag_range", (-3, 4)))
        for suffix, window in forms:
            for ab in ((), (True,)):
                tag = "abs" if ab else "default"
                _attempt(M, log, "run_rows%s(rows, %s)" % (suffix, tag), lambda: getattr(db, "run_rows" + suffix)(rows, *window, *ab))
                _attempt(M, log, "run_row_ptrs%s(series, %s)" % (suffix, tag),
                         lambda: getattr(db, "run_row_ptrs" + suffix)(series, *window, *ab))
                _attempt(M, log, "run_group_rows%s(src, idx, %s)" % (suffix, tag),
                         lambda: getattr(db, "run_group_rows" + suffix)(src, idx, *window, *ab))
            _attempt(M, log, "run_rows%s(row stride 16)" % suffix, lambda: getattr(db, "run_rows" + suffix)(wide, *window))
            _attempt(M, log, "run_rows%s(one row)" % suffix, lambda: getattr(db, "run_rows" + suffix)(rows[:1], *window))
            _attempt(M, log, "run_rows%s(no row)" % suffix, lambda: getattr(db, "run_rows" + suffix)(rows[:0], *window))
            _attempt(M, log, "run_rows%s(column stride 2: copied)" % suffix,
                     lambda: getattr(db, "run_rows" + suffix)(wide[:, ::2], *window))
            _attempt(M, log, "run_rows%s(1-D)" % suffix, lambda: getattr(db, "run_rows" + suffix)(rows[0], *window))
            _attempt(M, log, "run_row_ptrs%s(no series)" % suffix, lambda: getattr(db, "run_row_ptrs" + suffix)([], *window))
            _attempt(M, log, "run_row_ptrs%s(a series of 7)" % suffix,
                     lambda: getattr(db, "run_row_ptrs" + suffix)(series[:2] + [series[2][:7]], *window))
            _attempt(M, log, "run_row_ptrs%s(a 2-D series)" % suffix,
                     lambda: getattr(db, "run_row_ptrs" + suffix)([rows], *window))
            _attempt(M, log, "run_group_rows%s(src, list)" % suffix,
                     lambda: getattr(db, "run_group_rows" + suffix)(src, [2, 0, 3], *window))
            lib.fail_next = M.B.MUSE_ERR_LENGTH
            _attempt(M, log, "run_rows%s refused" % suffix, lambda: getattr(db, "run_rows" + suffix)(rows, *window))
        _attempt(M, log, "run_rows_windowed_scores(rows)", lambda: db.run_rows_windowed_scores(rows, 9))
        _attempt(M, log, "run_rows_windowed_scores(row stride 16)", lambda: db.run_rows_windowed_scores(wide, 9))
        _attempt(M, log, "run_rows_windowed_scores(1-D)", lambda: db.run_rows_windowed_scores(rows[0], 9))
        _attempt(M, log, "run_rows_in_lag_range_scores(rows)", lambda: db.run_rows_in_lag_range_scores(rows, -3, 4))
        _attempt(M, log, "run_rows_in_lag_range_scores(row stride 16)", lambda: db.run_rows_in_lag_range_scores(wide, -3, 4))
        _attempt(M, log, "run_rows_in_lag_range_scores(1-D)", lambda: db.run_rows_in_lag_range_scores(rows[0], -3, 4))

    # ---- module level: the many-references Runs (they marshal group_id too) and the plans
    log, lib, db = section("module level")
    with _patched(M, lib):
        db2 = _bare_batch(M, 0x5100, db.dgroup)
        for g in (None, gid):
            tag = "gid" if g is not None else "None"
            for name in ("run_many", "run_many_windowed", "run_many_in_window"):
                _attempt(M, log, "%s(%s)" % (name, tag), lambda: getattr(M, name)([db, db2], g, 3, 7, 5, 0.125, -1, False))
                _attempt(M, log, "%s(%s) defaults" % (name, tag), lambda: getattr(M, name)([db, db2], g))
            _attempt(M, log, "run_many_in_lag_range(%s)" % tag,
                     lambda: M.run_many_in_lag_range([db, db2], -3, 4, g, 3, 5, 0.125, -1, False))
            _attempt(M, log, "run_many_in_lag_range(%s) defaults" % tag, lambda: M.run_many_in_lag_range([db, db2], -3, 4, g))
        _attempt(M, log, "run_many(gid) top_n=0", lambda: M.run_many([db, db2], gid, 3, 7, 0))
        for f32 in (False, True):
            _attempt(M, log, "in_window_plan", lambda: M.in_window_plan(4096, f32, 64))
            _attempt(M, log, "lag_range_plan", lambda: M.lag_range_plan(4096, f32, -3, 4))
            _attempt(M, log, "signed_lag_range_plan", lambda: M.signed_lag_range_plan(4096, f32, -3, 4, -1))
            _attempt(M, log, "lag_band_plan", lambda: M.lag_band_plan(4096, f32, 1, 4, 1))
            _attempt(M, log, "lag_band_plan default", lambda: M.lag_band_plan(4096, f32, 1, 4))
            _attempt(M, log, "slide_in_window_plan", lambda: M.slide_in_window_plan(4096, f32, 64, 16))
            _attempt(M, log, "many_in_window_plan", lambda: M.many_in_window_plan(4096, f32, 64, 8))
            _attempt(M, log, "many_lag_range_plan", lambda: M.many_lag_range_plan(4096, f32, -3, 4, 8))
        for R in (0, 1, 3):
            _attempt(M, log, "window_many_plan(R=%d)" % R, lambda: M.window_many_plan(R, 7))
            _attempt(M, log, "window_many_plan_rows(R=%d)" % R, lambda: M.window_many_plan_rows(R, 15))
        _attempt(M, log, "window_rows_plan", lambda: M.window_rows_plan(16, 4096, 256))
        _attempt(M, log, "rows_lag_range_plan", lambda: M.rows_lag_range_plan(16, 4096, 256, -3, 4))
        lib.fail_next = M.B.MUSE_ERR_INVALID
        _attempt(M, log, "lag_band_plan refused", lambda: M.lag_band_plan(4096, False, 4, 1))
    return sections


# ------------------------------------------------------------------ level 2: the feeds
class _StubBatch:
    """stands in for a Batch's / Muse's DeviceBatch: logs the method and its arguments as the real method binds them"""

    def __init__(self, M, log, handle, canned):
        self._M, self._log, self._canned = M, log, canned
        self._h = ctypes.c_void_p(handle)
        self.dgroup = None

    def __getattr__(self, name):
        real = getattr(self._M.DeviceBatch, name)     # AttributeError: no such DeviceBatch method
        sig = inspect.signature(real)

        def method(*args, **kwargs):
            bound = sig.bind(self, *args, **kwargs)
            bound.apply_defaults()
            self._log.append("  DeviceBatch.%s(%s)" % (name, ", ".join(
                "%s=%s" % (k, self._arg(v)) for k, v in list(bound.arguments.items())[1:])))
            return self._canned(name, bound.arguments)
        return method

    @staticmethod
    def _arg(v):
        if isinstance(v, np.ndarray):
            return "%s%s%s" % (v.dtype.name, list(v.shape), [x.item() for x in v.reshape(-1)])
        if isinstance(v, _StubGroup):
            return "<group>"
        if isinstance(v, list):
            return "[" + ", ".join(_StubBatch._arg(x) for x in v) + "]"
        return _show(v)


def _results(M, log, tag, *settings):
    class Recording(M.Results):
        def Update(self, s):
            log.append("  %sUpdate(%s, Lag=%s, PercentScore=%s)" % (tag, s.Labels.ID() if s.Labels is not None else None,
                                                                   _show(s.Lag), _show(s.PercentScore)))
            return super().Update(s)
    return Recording(*settings)


def _fetch(log, results, tag=""):
    scores, mean = results.Fetch()
    log.append("  %sFetch -> [%s], %r" % (tag, ", ".join("%s %d %r" % (s.Labels.ID(), s.Lag, s.PercentScore) for s in scores), mean))


def _comparison(M, n_series=4):
    g = M.NewGroup("comparison")
    for i in range(n_series):
        g.Add(M.NewSeries(np.arange(8.0) + i, M.NewLabels({"two": "t%d" % (i % 2), "three": "h%d" % (i % 3), "uid": "s%d" % i})))
    return g


_SELECTION = {   # series index, lag, score: out of group order, both signs, one lag outside MaxLag = 5
    "idx": np.array([3, 0, 2, 1], dtype=np.int64), "lag": np.array([1, -2, 6, 0], dtype=np.int32),
    "score": np.array([0.9, -0.8, 0.7, -0.05])}


def _canned_selection(name, arguments):
    if name == "run_groups":
        G = arguments["G"]
        rec = np.zeros(G, dtype=[("series", "<i8"), ("score", "<f8"), ("lag", "<i4"), ("group", "<i4")])
        rec["series"], rec["score"], rec["lag"], rec["group"] = [1, 2, 0][:G], [0.5, -0.75, 0.25][:G], [0, -1, 2][:G], [0, 1, 2][:G]
        return rec, np.ones(G, dtype=np.uint8)
    if name == "set_lag_window":
        return None
    return _SELECTION["idx"].copy(), _SELECTION["lag"].copy(), _SELECTION["score"].copy(), 0.6125


def record_feeds(M):
    """level 2: {section: [lines]}"""
    sections = {}
    ANY, POS, NEG = M.SignFilter_ANY, M.SignFilter_POS, M.SignFilter_NEG
    engine = type("StubEngine", (), {"_reuse": True})()

    def batch(log, comp, sign, handle=0x7000, max_lag=5, engines=None, tag=""):
        b = object.__new__(M.Batch)
        b.Concurrency, b.Comparison, b.Results = 1, comp, _results(M, log, tag, max_lag, 5, 0.1, sign)
        b._engines, b._engine, b._ref, b._db, b._shard_db, b.n = engines, engine, np.arange(8.0), None, None, 8
        stub = _StubBatch(M, log, handle, _canned_selection)
        b._batch = lambda: stub
        return b

    runs = (("Run", ()), ("RunWindowed", ()), ("RunInWindow", ()), ("RunInLagRange", (-3, 4)), ("RunSignedInLagRange", (-3, 4)),
            ("RunInLagBand", (1, 4)), ("RunSignedInLagBand", (1, 4)), ("RunSigned", ()))
    bad = {"RunInWindow": dict(max_lag=-1), "RunSigned": dict(max_lag=-1), "RunInLagRange": dict(args=(1, 4)),
           "RunSignedInLagRange": dict(args=(-3, -1)), "RunInLagBand": dict(args=(4, 1)), "RunSignedInLagBand": dict(args=(4, 1))}

    log = sections["Batch feeds"] = []
    lib = RecordingLib(M, log)             # (Batch.Run's exact feed merges its winners through the C library)
    with _patched(M, lib):
        M.EXACT_FEED_MAX_GROUPS = 2
        comp = _comparison(M)
        for name, args in runs:
            for by in (["two"], ["three"]):    # 2 label groups: the exact feed; 3: beyond EXACT_FEED_MAX_GROUPS
                for sign in (ANY, POS, NEG):
                    b = batch(log, comp, sign)
                    _attempt(M, log, "Batch.%s(%s%s), SignFilter %d" % (name, by, "".join(", %d" % a for a in args), sign),
                             lambda: getattr(b, name)(list(by), *args))
                    _fetch(log, b.Results)

    log = sections["Batch refusals"] = []
    lib = RecordingLib(M, log)
    with _patched(M, lib):
        M.EXACT_FEED_MAX_GROUPS = 2
        comp, empty = _comparison(M), M.NewGroup("empty")
        for name, args in runs:
            how = bad.get(name, {})
            bad_args = how.get("args", args)
            # an empty label set wins over everything, a sharded batch over the method's own argument check
            b = batch(log, empty, POS, engines=[engine, engine], max_lag=how.get("max_lag", 5))
            _attempt(M, log, "Batch.%s: empty, sharded, bad arguments" % name, lambda: getattr(b, name)(["two"], *bad_args))
            if name in ("Run", "RunWindowed"):
                continue                       # (they run sharded)
            b = batch(log, comp, POS, engines=[engine, engine], max_lag=how.get("max_lag", 5))
            _attempt(M, log, "Batch.%s: sharded, bad arguments" % name, lambda: getattr(b, name)(["two"], *bad_args))
            b = batch(log, comp, POS, max_lag=how.get("max_lag", 5))
            _attempt(M, log, "Batch.%s: bad arguments" % name, lambda: getattr(b, name)(["two"], *bad_args))
            b = batch(log, comp, POS, engines=[engine, engine])
            _attempt(M, log, "Batch.%s: sharded" % name, lambda: getattr(b, name)(["two"], *args))

    log = sections["RunMany feeds"] = []
    lib = RecordingLib(M, log)
    with _patched(M, lib):
        M.EXACT_FEED_MAX_GROUPS = 2
        comp = _comparison(M)
        many = (("RunMany", ()), ("RunManyWindowed", ()), ("RunManyInWindow", ()), ("RunManyInLagRange", (-3, 4)))
        for name, args in many:
            for by in (["two"], ["three"]):
                for sign in (ANY, NEG):
                    bs = [batch(log, comp, sign, 0x7000 + 0x100 * i, tag="[%d] " % i) for i in range(2)]
                    _attempt(M, log, "%s(%s%s), SignFilter %d" % (name, by, "".join(", %d" % a for a in args), sign),
                             lambda: getattr(M, name)(bs, list(by), *args))
                    for i, b in enumerate(bs):
                        _fetch(log, b.Results, "[%d] " % i)
            # Results settings that differ: each batch takes its own method
            bs = [batch(log, comp, (ANY, POS)[i], 0x7000 + 0x100 * i, tag="[%d] " % i) for i in range(2)]
            _attempt(M, log, "%s: settings differ" % name, lambda: getattr(M, name)(bs, ["three"], *args))
            _attempt(M, log, "%s: no batch" % name, lambda: getattr(M, name)([], ["three"], *args))
        bs = [batch(log, comp, ANY, 0x7000 + 0x100 * i, max_lag=-1) for i in range(2)]
        _attempt(M, log, "RunManyInWindow: MaxLag -1", lambda: M.RunManyInWindow(bs, ["two"]))
        _attempt(M, log, "RunManyInLagRange: bad range", lambda: M.RunManyInLagRange(bs, ["two"], 1, 4))

    # ---- Muse
    log = sections["Muse"] = []
    lib = RecordingLib(M, log)
    with _patched(M, lib):
        home = _StubGroup(8, 10, engine)
        other = _StubGroup(8, 10, engine)

        def graphs(n=3, resident=None, short=None):
            out = []
            for i in range(n):
                s = M.NewSeries(np.arange(7.0 if i == short else 8.0) + i, M.NewLabels({"uid": "g%d" % i}))
                if resident is not None:
                    s._home = (weakref.ref(resident[i] if isinstance(resident, list) else resident), 2 * i + 1, 0)
                out.append(s)
            return out

        def muse(max_lag=5, winner=(1, -2, 0.75), state=1, reuse=True, bare=False):
            m = object.__new__(M.Muse)
            m.refN, m.n, m._ref = 8, 8, np.arange(8.0)
            m.Results = _results(M, log, "", max_lag, 5, 0.1, ANY)
            m._engine = engine
            engine._reuse = reuse

            def canned(name, arguments):
                rec = np.zeros(1, dtype=[("series", "<i8"), ("score", "<f8"), ("lag", "<i4"), ("group", "<i4")])
                rec["series"], rec["lag"], rec["score"] = winner
                return rec[0], state
            if not bare:     # (bare: a refusal comes before anything touches the device side)
                m._template = _StubBatch(M, log, 0x7000, canned)
            return m

        forms = (("Run", (), {}), ("RunWindowed", (), {}), ("RunWindowed", (), dict(max_lag=64)), ("RunWindowed", (), dict(max_lag=-1)),
                 ("RunInLagRange", (-3, 4), {}), ("RunInLagRange", (1, 4), {}), ("RunInLagRange", (-3, -1), {}))
        for name, args, how in forms:
            tag = "Muse.%s(%s)%s" % (name, ", ".join(str(a) for a in args), " MaxLag %d" % how["max_lag"] if how else "")
            if not how and args in ((), (-3, 4)):
                _attempt(M, log, tag + ": host rows", lambda: getattr(muse(), name)(graphs(), *args))
                _attempt(M, log, tag + ": resident rows", lambda: getattr(muse(), name)(graphs(resident=home), *args))
                _attempt(M, log, tag + ": resident rows, reuse off", lambda: getattr(muse(reuse=False), name)(graphs(resident=home), *args))
                _attempt(M, log, tag + ": rows resident in two groups",
                         lambda: getattr(muse(), name)(graphs(resident=[home, other, home]), *args))
                _attempt(M, log, tag + ": no member (state 0)", lambda: getattr(muse(state=0), name)(graphs(), *args))
                _attempt(M, log, tag + ": NaN group (state 2)", lambda: getattr(muse(state=2), name)(graphs(), *args))
                _attempt(M, log, tag + ": winner -1", lambda: getattr(muse(winner=(-1, 0, 0.0)), name)(graphs(), *args))
                _attempt(M, log, tag + ": winner outside MaxLag", lambda: getattr(muse(winner=(2, 6, 0.5)), name)(graphs(), *args))
            # the order of the refusals: nothing for an empty list; the method's own bound before the length check
            _attempt(M, log, tag + ": empty list", lambda: getattr(muse(bare=True, **how), name)([], *args))
            _attempt(M, log, tag + ": a series of 7", lambda: getattr(muse(bare=True, **how), name)(graphs(short=1), *args))
        m = muse(max_lag=63)
        _attempt(M, log, "Muse.RunWindowed() MaxLag 63", lambda: m.RunWindowed(graphs()))
        _fetch(log, m.Results)
        engine._reuse = True
    return sections


# ------------------------------------------------------------------ signatures
def record_signatures(M):
    def entry(obj):
        doc = inspect.getdoc(obj)
        return "%s doc:%s" % (inspect.signature(obj), hashlib.sha1(doc.encode()).hexdigest()[:12] if doc else "-")
    out = {}
    for name, obj in sorted(vars(M).items()):
        if name.startswith("_") or getattr(obj, "__module__", None) != M.__name__ or not callable(obj):
            continue
        out[name] = entry(obj)
    for cls in (M.DeviceBatch, M.Batch, M.Muse):
        for name, obj in sorted(vars(cls).items()):
            if name.startswith("_") or not callable(getattr(cls, name)):
                continue
            out["%s.%s" % (cls.__name__, name)] = entry(getattr(cls, name))
    return out


def record():
    M = pkg().muse
    calls = record_c_calls(M)
    calls.update(record_feeds(M))
    return {"signatures": record_signatures(M), "calls": calls}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    rec = record()
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=False)
            f.write("\n")
        print("wrote %s: %d signatures, %d lines" % (FIXTURE, len(rec["signatures"]), sum(len(v) for v in rec["calls"].values())))
    else:
        json.dump(rec, sys.stdout, indent=1)
