"""CPU-only checks of muse_group_slide (rows of a resident group moved forward in time, in place): the export and its test hook
exist on every layer (headers, library, binding), the kernel's vector unit is the widest that both the row length and the shift
allow, and a Series' home in a DeviceGroup dies with the group's next slide."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _load import ROOT, pkg


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(muse_[a-z0-9_]+)\s*\(", hdr))


def test_exports_declared_exported_and_bound(muse):
    assert "muse_group_slide" in _declared("muse_hip.h")
    assert "muse_test_slide_plan" in _declared("muse_hip_test.h")
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for name in ("muse_group_slide", "muse_test_slide_plan"):
        assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
        assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    assert len(muse.binding.SIGNATURES["muse_group_slide"][1]) == 6
    # an addition: the ABI version stays
    assert muse.binding.load().muse_abi_version() == 5


def _unit(muse, N, k, f32):
    u = ctypes.c_int32(-1)
    rc = muse.binding.load().muse_test_slide_plan(N, k, 1 if f32 else 0, ctypes.byref(u))
    return rc, int(u.value)


@pytest.mark.parametrize("f32,N,k,unit", [
    (False, 4096, 2, 16), (False, 4096, 1, 8), (False, 4095, 2, 8), (False, 4096, 4096, 16),
    (True, 4096, 4, 16), (True, 4096, 2, 8), (True, 4096, 1, 4), (True, 4097, 4, 4),
])
def test_slide_plan_unit(muse, f32, N, k, unit):
    assert _unit(muse, N, k, f32) == (0, unit)


def test_slide_plan_unit_divides_both_offsets(muse):
    """the rule itself, over a sweep: the unit divides N x elem and k x elem, and no wider unit of 16 / 8 / 4 does"""
    for f32 in (False, True):
        elem = 4 if f32 else 8
        for N in (1, 2, 3, 7, 8, 255, 256, 480, 1433, 4095, 4096, 4097, 70000, 1 << 20):
            for k in sorted({0, 1, 2, 3, 4, 6, 8, N // 2, max(N - 1, 0), N}):
                if k > N:
                    continue
                rc, u = _unit(muse, N, k, f32)
                assert rc == 0 and u in (4, 8, 16) and u >= elem, (f32, N, k, u)
                assert (N * elem) % u == 0 and (k * elem) % u == 0, (f32, N, k, u)
                if u < 16:
                    assert (N * elem) % (2 * u) or (k * elem) % (2 * u), (f32, N, k, u)


def test_slide_plan_refuses_bad_arguments(muse):
    E = muse.binding.MUSE_ERR_INVALID
    assert _unit(muse, 0, 0, False)[0] == E
    assert _unit(muse, 8, -1, False)[0] == E
    assert _unit(muse, 8, 9, False)[0] == E
    assert muse.binding.load().muse_test_slide_plan(8, 1, 0, None) == E


def test_slide_refuses_a_null_group_without_a_device(muse):
    t = np.zeros(4)
    rc = muse.binding.load().muse_group_slide(None, 0, 1, muse.binding.dptr(t), 4, 4)
    assert rc == muse.binding.MUSE_ERR_INVALID


# ------------------------------------------------------------------ the mirror: a home dies with the group's next slide
class _Engine:
    pass


class _FakeGroup:
    def __init__(self, engine, N, slides=None):
        self.engine, self.N, self.f32, self.alive = engine, N, False, True
        if slides is not None:
            self.slides = slides


def test_home_set_before_a_slide_is_dead_afterwards(muse):
    m = muse.muse
    eng = _Engine()
    g = _FakeGroup(eng, 8, slides=0)
    a, b = muse.NewSeries(np.zeros(8)), muse.NewSeries(np.zeros(8))
    m.set_home(a, g, 3)
    assert m.live_home(a, eng, 8) == (g, 3)
    g.slides += 1
    assert m.live_home(a, eng, 8) is None
    assert m.plan_rows([a], eng, 8) == [("host", 0, 1)]
    m.set_home(b, g, 4)                      # set after the slide: live
    assert m.live_home(b, eng, 8) == (g, 4)
    g.slides += 1
    assert m.live_home(b, eng, 8) is None


def test_a_home_that_slid_away_is_replaced(muse):
    m = muse.muse
    eng = _Engine()
    g, h = _FakeGroup(eng, 8, slides=2), _FakeGroup(eng, 8, slides=0)
    s = muse.NewSeries(np.zeros(8))
    m.set_home(s, g, 1)
    m.set_home(s, h, 5)                      # the first home is kept while it holds the values
    assert m.live_home(s, eng, 8) == (g, 1)
    g.slides = 3
    m.set_home(s, h, 5)
    assert m.live_home(s, eng, 8) == (h, 5)


def test_a_group_without_a_slide_counter_behaves_as_before(muse):
    m = muse.muse
    eng = _Engine()
    g = _FakeGroup(eng, 8)
    assert not hasattr(g, "slides")
    s = muse.NewSeries(np.zeros(8))
    m.set_home(s, g, 2)
    assert m.live_home(s, eng, 8) == (g, 2)
    g.alive = False
    assert m.live_home(s, eng, 8) is None


def test_device_group_has_slide():
    m = pkg().muse
    assert hasattr(m.DeviceGroup, "slide")
