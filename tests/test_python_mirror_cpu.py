"""go-muse_amd/muse.py against its recorded calls (no device, no built library): which C function every DeviceBatch wrapper and
plan function calls and with what arguments, what Batch / Muse / RunMany* ask of the device side and feed to Results.Update and
in what order, every refusal's status and message, and the signature and docstring of every public name.  The record
(tests/golden/python_mirror_calls.json; tests/_mirrorlog.py wrote it and says how) was taken before the wrappers were factored
onto shared cores, so a change of muse.py that alters none of its lines changed the code's shape, not what it does."""
import pytest

import _mirrorlog as ML

GOLDEN = ML.load_fixture()


@pytest.fixture(scope="module")
def recorded():
    return ML.record()


def test_fixture_holds_both_levels_and_the_signatures():
    assert set(GOLDEN) == {"signatures", "calls"}
    assert {"DeviceBatch selection", "DeviceBatch slide", "DeviceBatch winner", "module level", "Batch feeds", "Batch refusals",
            "RunMany feeds", "Muse"} == set(GOLDEN["calls"])
    assert all(len(lines) > 20 for lines in GOLDEN["calls"].values())


def test_same_sections(recorded):
    assert list(recorded["calls"]) == list(GOLDEN["calls"])


@pytest.mark.parametrize("section", list(GOLDEN["calls"]))
def test_calls_line_by_line(recorded, section):
    got, want = recorded["calls"][section], GOLDEN["calls"][section]
    label = ""
    for k, (g, w) in enumerate(zip(got, want)):
        if w.startswith("> "):
            label = w
        assert g == w, "%s, line %d (%s)" % (section, k, label)
    assert len(got) == len(want), "%s: %d lines recorded, %d expected; the first one over: %r" % (
        section, len(got), len(want), (got + want)[min(len(got), len(want))])


def test_signatures_and_docstrings(recorded):
    got, want = recorded["signatures"], GOLDEN["signatures"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_recording_leaves_the_module_as_it_was(recorded):
    M = ML.pkg().muse
    assert M.EXACT_FEED_MAX_GROUPS == 65536
    assert M.B.load.__module__ == M.B.__name__
