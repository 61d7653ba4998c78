"""Host-side checks of the adaptive split-scale mode (include/umetrack_hip.h: UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE): the
Python binding's mode names and scoping, the exported entry, and the header's C99 declarations.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import pytest

from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeLib:
    """Records the ut_set_split_scale / ut_get_split_adaptations calls of a HipEngine built without a device."""

    def __init__(self):
        self.calls = []
        self.count = 7

    def ut_set_split_scale(self, h, mode):
        self.calls.append(("set", mode))
        return 0

    def ut_get_split_adaptations(self, h, out, reset, stream):
        out._obj.value = self.count
        self.calls.append(("get", reset))
        if reset:
            self.count = 0
        return 0

    def ut_destroy(self, h):
        return 0


def _engine(monkeypatch):
    eng = object.__new__(_native.HipEngine)
    eng.lib = _FakeLib()
    eng._h = ctypes.c_void_p(1)
    eng.device = None
    eng.deferred_checks = False
    eng.latency_mode = False
    eng.split_scale = "calibrated"
    monkeypatch.setattr(_native, "_stream", lambda d: None)
    return eng


def test_split_scale_names_map_to_the_c_modes(monkeypatch):
    eng = _engine(monkeypatch)
    for name, mode in (("adaptive", 2), ("dynamic", 1), ("calibrated", 0)):
        eng.set_split_scale(name)
        assert eng.lib.calls[-1] == ("set", mode) and eng.split_scale == name
    n = len(eng.lib.calls)
    for bad in ("Adaptive", "calibrated_adaptive", "auto", ""):
        with pytest.raises(KeyError):
            eng.set_split_scale(bad)
    assert len(eng.lib.calls) == n and eng.split_scale == "calibrated"
    eng._h = None


def test_modes_scopes_the_split_scale_and_puts_it_back(monkeypatch):
    eng = _engine(monkeypatch)
    with eng.modes(split_scale="adaptive"):
        assert eng.split_scale == "adaptive"
    assert eng.split_scale == "calibrated"
    assert [c for c in eng.lib.calls if c[0] == "set"] == [("set", 2), ("set", 0)]
    eng.set_split_scale("dynamic")
    eng.lib.calls.clear()
    with pytest.raises(RuntimeError):
        with eng.modes(split_scale="adaptive"):
            raise RuntimeError("inside")
    assert eng.split_scale == "dynamic" and eng.lib.calls == [("set", 2), ("set", 1)]
    eng.lib.calls.clear()
    with eng.modes(split_scale="dynamic"):          # already set: no call either way
        pass
    assert eng.lib.calls == []
    eng._h = None


def test_split_adaptations_reads_and_resets(monkeypatch):
    eng = _engine(monkeypatch)
    assert eng.split_adaptations() == 7
    assert eng.split_adaptations(reset=True) == 7
    assert eng.split_adaptations() == 0
    assert eng.lib.calls == [("get", 0), ("get", 1), ("get", 0)]
    eng._h = None


def test_library_exports_the_adaptations_entry():
    assert "ut_get_split_adaptations" in _native.EXPORTS
    lib = ctypes.CDLL(_native.LIB_PATH)          # (built by build(); loading it needs no device)
    assert lib.ut_get_split_adaptations
    # argument validation only: a null handle is refused without touching a device
    assert lib.ut_get_split_adaptations(None, None, 0, None) < 0
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        assert " ut_get_split_adaptations" in out.stdout


def test_header_declares_the_adaptive_mode_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "split_adaptive_c99.c"), "-o", str(tmp_path / "split_adaptive.o")])
