"""The generator and the model of the state sequences (tests/_seq.py) on their own: no device.  What the GPU test
(tests/test_gpu_state_sequences.py) relies on is asserted here of the COMMITTED seeds: the sequences are deterministic, every
operation is emitted in a state that allows it, the sequences of a class hold every (mutator or setting -> reader) pair, every refusal
occurs, and no state they pass through has tied continuous-noise rows (so a lag that differs from the oracle's is a finding, not a
tie)."""
import json

import numpy as np
import pytest

import _seq
import _window as W

ALL = [(cls, seed) for cls in _seq.CLASSES for seed in _seq.SEEDS[cls]]


@pytest.fixture(scope="module")
def sequences():
    return {cs: _seq.generate(*cs) for cs in ALL}


def test_the_generator_is_deterministic_per_seed(sequences):
    for (cls, seed), ops in sequences.items():
        again = _seq.generate(cls, seed)
        assert json.dumps(again) == json.dumps(ops), (cls, seed)        # (and the list survives the round trip a replay takes)
        assert json.loads(json.dumps(ops)) == ops
        assert len(ops) == _seq.CLASSES[cls]["steps"]
    for cls in _seq.CLASSES:
        a, b = (sequences[(cls, s)] for s in _seq.SEEDS[cls])
        assert a != b
    m1, m2 = _seq.Model("b", 1), _seq.Model("b", 1)
    assert m1.rows.tobytes() == m2.rows.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(m1.refs, m2.refs))
    assert _seq.Model("b", 2).rows.tobytes() != m1.rows.tobytes()


def test_class_limits(sequences):
    """the issue's table: about 40 steps for a to e, at most 12 and one windowed reader for g"""
    for cls in "abcde":                                                  # (class a: its scripted cache stretches come on top)
        assert 40 <= _seq.CLASSES[cls]["steps"] <= 50
    assert _seq.CLASSES["g"]["steps"] <= 12 and _seq.CLASSES["g"]["wcap"] == 1
    for (cls, seed), ops in sequences.items():
        if cls == "g":
            n = 0
            for m, op, d, ok in _seq.walk(cls, seed, ops):
                n += m.windowed_reader(op)
            assert n <= 1, (seed, n)


def test_every_precondition_holds_where_the_operation_is_emitted(sequences):
    for (cls, seed), ops in sequences.items():
        last = None
        for i, (m, op, d, ok) in enumerate(_seq.walk(cls, seed, ops)):
            assert ok, (cls, seed, i, op)
            # the model itself: a float32 group holds float32 values, the row kinds follow the rows
            assert len(m.kinds) == m.M and m.rows.shape[1] == m.shape.N
            if m.shape.f32:
                assert m.rows.tobytes() == _seq.stored(m.rows, True).tobytes()
            assert sum(k in ("copy", "neg") for k in m.kinds) <= 1
            if last is not None and _seq.GROUP[last["kind"]] == "refusal":
                assert _seq.GROUP[op["kind"]] == "reader", (cls, seed, i)    # the next reader is checked like any other
            last = op


def test_the_model_slides_and_appends_as_numpy_says():
    m = _seq.Model("e", 3)
    before = m.rows.copy()
    op = dict(kind="slide", first=3, count=5, k=16, dseed=9)
    assert m.precondition(op)
    d = m.prepare(op)
    m.apply(op, d)
    want = before.copy()
    want[3:8] = np.concatenate([before[3:8, 16:], d["tails"].astype(np.float32).astype(np.float64)], 1)
    assert m.rows.tobytes() == want.tobytes() and m.version == 1 and m.slides == 1
    op = dict(kind="append", how="small", count=9, dseed=4)
    d = m.prepare(op)
    m.apply(op, d)
    assert m.M == before.shape[0] + 9 and m.rows[:before.shape[0]].tobytes() == want.tobytes()
    assert m.kinds[-9:][3:7] == ["const", "nan", "inf", "mean"] and np.isnan(m.rows[-5]).sum() == 1
    assert not m.precondition(dict(kind="slide", first=0, count=m.M + 1, k=1, dseed=1))
    assert not m.precondition(dict(kind="window", j=0, L=7))            # a float32 group: the refusal, not the setting
    assert m.precondition(dict(kind="refuse_window_f32", j=0, L=7))


# ------------------------------------------------------------------ coverage of the committed seeds
def test_every_pair_of_mutator_or_setting_and_reader_occurs_in_every_class(sequences):
    """for every class, every applicable ordered pair (mutator or setting kind -> reader kind) with no other mutator between the two,
    in at least one committed sequence of that class.  The kinds are the bullets of the operation list (_seq.FAMILY).  Class g is held
    to what its 12 steps can hold: 2 x 12 steps cannot contain 10 kinds x 6 readers -- every pair of a slide (plain or fused) and
    the three readers whose kernel selection it must reset (scores, run, run_groups), and every reader kind at all.  A reader counts
    only if it reads this group: a Muse.Run over host rows or over the other group never meets the state the mutator left."""
    for cls in _seq.CLASSES:
        muts, sets = _seq.applicable_families(cls)
        have = set()
        for seed in _seq.SEEDS[cls]:
            have |= _seq.pairs_of(sequences[(cls, seed)])
        if cls == "g":
            want = {(a, r) for a in ("slide", "slide_score") for r in ("scores", "run", "run_groups")}
            assert {r for _, r in have} == set(_seq.READER_FAMILIES)
        else:
            want = {(a, r) for a in muts + sets for r in _seq.READER_FAMILIES}
        assert not (want - have), (cls, sorted(want - have))


def test_every_refusal_and_every_operation_kind_occurs(sequences):
    kinds = {op["kind"] for ops in sequences.values() for op in ops}
    assert set(_seq.REFUSALS) <= kinds, set(_seq.REFUSALS) - kinds
    assert set(_seq.GROUP) <= kinds, set(_seq.GROUP) - kinds
    hows = {op["how"] for ops in sequences.values() for op in ops if op["kind"] == "append"}
    assert hows == {"one", "small", "slab"}
    for cls in _seq.CLASSES:                                             # slides of the whole group and of a sub-range, every k
        sl = [op for seed in _seq.SEEDS[cls] for op in sequences[(cls, seed)] if op["kind"] == "slide"]
        assert any(op["first"] > 0 for op in sl), cls
    for seed in _seq.SEEDS["f"]:                                         # (the kept statistics: every sequence of the class)
        assert any(op["kind"] == "slide" and op["first"] > 0 for op in sequences[("f", seed)]), seed
    # the slide widths of the issue's list -- 1, 2, 3, 16, 65, N // 2, N -- all occur (a class of 40 steps holds a handful of slides)
    ks = {"half" if op["k"] == _seq.CLASSES[cls]["N"] // 2 else "all" if op["k"] == _seq.CLASSES[cls]["N"] else op["k"]
          for (cls, seed), ops in sequences.items() for op in ops if op["kind"] in ("slide", "slide_score", "slide_run")}
    assert ks == {1, 2, 3, 16, 65, "half", "all"}, ks
    ls = {op["L"] for ops in sequences.values() for op in ops if op["kind"] == "window"}
    assert ls == set(_seq.WINDOWS)


def test_the_states_the_suite_cannot_reach_otherwise_occur(sequences):
    """a screened Run in every sequence that switches screening on; a packed many-references pass followed by a fused slide of one of
    its batches with no other scoring pass of that batch between (muse_batch::origin, PACKED); a slide between two unwindowed passes of
    one batch (the spectrum cache in class a, the kept statistics in class f, the learned hand-off in class g)"""
    stale_tiles, slid = 0, set()
    for (cls, seed), ops in sequences.items():
        # passes that count towards the group's spectrum cache (the second one builds it); what happened to a BUILT cache since the
        # last such pass; the (event -> pass) stretches the sequence holds
        built, pending, cache_stretches = 0, set(), set()
        s = _seq.Shape(cls)
        switched, eligible = False, 0
        packed = set()
        state = {}             # batch -> "scored" (an unwindowed pass over the rows as they are) | "slid" (... and the rows slid since)
        slid_between = False
        for m, op, d, ok in _seq.walk(cls, seed, ops):
            k = op["kind"]
            if k == "screening" and op["on"]:
                switched = True
            if k == "run" and m.screen_eligible(op):
                eligible += 1
            if k in ("scores_many_w", "run_many_w") and len(op["js"]) >= 2 and op["L"] <= 16:
                packed = set(op["js"])
            elif k in ("slide_score", "slide_run"):
                stale_tiles += op["j"] in packed
                packed.discard(op["j"])
            elif k in ("scores", "run", "run_groups"):
                packed.discard(op["j"])
            elif k in ("scores_many", "run_many"):
                packed -= set(op["js"])
            if k in ("scores", "run", "run_groups") and m.windows[op["j"]] < 0:
                slid_between = slid_between or state.get(op["j"]) == "slid"
                state[op["j"]] = "scored"
            if k in ("slide", "slide_score", "slide_run"):
                state = {j: "slid" for j in state}
            # the spectrum cache as DESIGN 4.10 describes it: limits lowered, an unwindowed fp64 pass of one batch counts, the second builds
            if s.cache:
                if k in ("scores", "run", "run_groups") and m.windows[op["j"]] < 0 and m.cache_limits and \
                        not (k == "run" and m.screen_eligible(op)):
                    cache_stretches |= pending
                    pending = set()
                    built += 1
                elif k in ("slide", "slide_score", "slide_run"):
                    pending, built = ({"slide"} if built >= 2 else set()), 0
                elif k in ("append", "stage_commit", "append_from", "refuse_slide_staged") and built >= 2:
                    pending.add("append")
                elif k == "drop_cache":
                    pending, built = ({"drop"} if built >= 2 else set()), 0
        if cls == "a":     # every sequence of the class: a pass right behind a slide under, an append to and a drop of a BUILT cache
            assert cache_stretches == {"slide", "append", "drop"}, (seed, cache_stretches)
        if switched and s.screen_ok:
            assert eligible >= 1, (cls, seed)
        if slid_between:
            slid.add(cls)
    assert set("afg") <= slid, slid
    assert stale_tiles >= 1


# ------------------------------------------------------------------ the oracle alone: no ties, and the block form of the window
def test_the_block_form_of_the_window_is_the_definition(oracle):
    N, M = 480, 40
    ref, rows = W.make_case(N, M, seed=5)
    Ls = (0, 7, 15, 16, 63)
    exp, glag, gmv, n = W.expect(oracle, ref, rows, Ls)
    e = _seq.Expect(oracle, [ref], n)
    for L in Ls:
        lag, mv, tie = e.windowed(0, rows, L)
        assert np.array_equal(lag, exp[L][0]) and mv.tobytes() == exp[L][1].tobytes() and np.array_equal(tie, exp[L][2]), L
        for r in (0, 1, 3, 4, 5, 6, 17):                                # (and the scalar definition itself: strict '>' in scan order)
            cc = oracle.xcorr_with_x(oracle.ref_spectrum(ref)[0], rows[r], n)[0]
            one = W.windowed(cc, n, L)
            assert (one[0], one[2]) == (int(lag[r]), bool(tie[r])) and (one[1] == mv[r] or (np.isnan(one[1]) and np.isnan(mv[r])))
    olag, omv, gap = oracle.batch_scores(ref, rows)
    lag, mv, g = e.scores(0, rows)
    assert np.array_equal(lag, olag) and mv.tobytes() == omv.tobytes() and g.tobytes() == gap.tobytes()
    # rows the cache has seen cost nothing and give the same
    again = e.windowed(0, rows[::-1].copy(), 7)
    assert np.array_equal(again[0], e.windowed(0, rows, 7)[0][::-1])


@pytest.mark.parametrize("cls,seed", ALL)
def test_no_state_has_tied_continuous_noise_rows(oracle, sequences, cls, seed):
    """every state a committed sequence passes through, every reference, without a window and at every window the class can set:
    the row generator by itself yields no tie.  Sampled where the full check is slow: class f (131072-point transforms) takes the
    first state and every third one after it, class g (2100 rows x 4096) checks the windows against its first reference only."""
    s = _seq.Shape(cls)
    sample = 3 if cls == "f" else 1
    seen, e, states = None, None, 0
    for m, op, d, ok in _seq.walk(cls, seed, sequences[(cls, seed)]):
        if e is None:
            e = _seq.Expect(oracle, m.refs, s.n)
        if m.version == seen:
            continue
        seen = m.version
        states += 1
        if (states - 1) % sample:
            continue
        keep = m.keep()
        for j in range(m.R):
            lag, mv, gap = e.scores(j, m.rows)
            tie = (gap < W.TIE_GAP) & ~np.isnan(mv) & keep
            assert not tie.any(), (cls, seed, states, j, np.flatnonzero(tie)[:4])
            if s.window_ok and (cls != "g" or j == 0):
                for L in e.LS:
                    assert not (e.windowed(j, m.rows, L)[2] & keep).any(), (cls, seed, states, j, L)
        e.forget(m.rows)
    assert states >= 2
