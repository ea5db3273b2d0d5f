"""CPU-only checks of the resident-row feature: the two exports exist on every layer (header, library, binding), and the
planning step of the host mirror (which series of a new Group are taken from a DeviceGroup that already holds them, which
go up from the host) keeps order and falls back to the host wherever a home does not fit."""
import ctypes
import os
import re
import subprocess

import pytest

from _load import ROOT, pkg

EXPORTS = ("muse_group_append_from", "muse_batch_run_group_rows")


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def test_exports_declared_exported_and_bound(muse):
    hdr = open(os.path.join(ROOT, "include", "muse_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), "muse_hip.h does not declare %s" % name
        assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
        assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    # backward compatible additions: the ABI version stays
    assert muse.binding.load().muse_abi_version() == 5


class _Engine:
    pass


class _FakeGroup:
    """what the planner looks at in a DeviceGroup: engine, N, storage type, liveness"""

    def __init__(self, engine, N, f32=False):
        self.engine, self.N, self.f32, self.alive = engine, N, f32, True


def _series(muse, n):
    import numpy as np
    return [muse.NewSeries(np.zeros(8)) for _ in range(n)]


def test_plan_runs_split_at_home_changes(muse):
    m = muse.muse
    eng = _Engine()
    a, b = _FakeGroup(eng, 8), _FakeGroup(eng, 8)
    ser = _series(muse, 7)
    m.set_home(ser[0], a, 5)
    m.set_home(ser[1], a, 2)
    m.set_home(ser[2], b, 0)
    # ser[3] has no home
    m.set_home(ser[4], a, 7)
    m.set_home(ser[5], a, 7)        # duplicates are fine
    m.set_home(ser[6], b, 1)
    runs = m.plan_rows(ser, eng, 8)
    assert [(r[0], r[1], r[2]) for r in runs] == [("device", 0, 2), ("device", 2, 3), ("host", 3, 4), ("device", 4, 6),
                                                  ("device", 6, 7)]
    assert runs[0][3] is a and list(runs[0][4]) == [5, 2]
    assert runs[1][3] is b and list(runs[1][4]) == [0]
    assert runs[3][3] is a and list(runs[3][4]) == [7, 7]
    assert runs[4][3] is b and list(runs[4][4]) == [1]
    # the runs cover the list in order, without gaps
    assert [r[1] for r in runs] == [0] + [r[2] for r in runs[:-1]] and runs[-1][2] == len(ser)


def test_plan_first_home_is_kept(muse):
    m = muse.muse
    eng = _Engine()
    a, b = _FakeGroup(eng, 8), _FakeGroup(eng, 8)
    s = _series(muse, 1)
    m.set_home(s[0], a, 3)
    m.set_home(s[0], b, 9)
    assert m.live_home(s[0], eng, 8) == (a, 3)


@pytest.mark.parametrize("why", ["dead", "collected", "engine", "N", "storage", "dst"])
def test_plan_falls_back_to_the_host(muse, why):
    m = muse.muse
    eng, other = _Engine(), _Engine()
    g = _FakeGroup(other if why == "engine" else eng, 9 if why == "N" else 8, f32=(why == "storage"))
    ser = _series(muse, 3)
    for i, s in enumerate(ser):
        m.set_home(s, g, i)
    if why == "dead":
        g.alive = False
    if why == "collected":
        del g
        import gc
        gc.collect()
        g = None
    runs = m.plan_rows(ser, eng, 8, False, dst=g if why == "dst" else None)
    assert runs == [("host", 0, 3)]


def test_plan_mixed_and_empty(muse):
    m = muse.muse
    eng = _Engine()
    live, dead = _FakeGroup(eng, 8), _FakeGroup(eng, 8)
    dead.alive = False
    ser = _series(muse, 5)
    m.set_home(ser[1], live, 4)
    m.set_home(ser[2], dead, 0)
    m.set_home(ser[3], live, 1)
    runs = m.plan_rows(ser, eng, 8)
    assert [(r[0], r[1], r[2]) for r in runs] == [("host", 0, 1), ("device", 1, 2), ("host", 2, 3), ("device", 3, 4),
                                                  ("host", 4, 5)]
    assert m.plan_rows([], eng, 8) == []


def test_reuse_switch_exists():
    """the Engine's A/B switch (creating an engine needs a device: the GPU suite checks that it is on by default)"""
    m = pkg().muse
    assert hasattr(m.Engine, "reuse_resident_rows")
