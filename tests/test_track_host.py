"""CPU tests of the sequences tracked in one launch (ut_track_pose_views, include/umetrack_hip_track.h): the C boundary, and the
float64 restatement of tests/track_cases.py - it is start_cases.track on the documented loss and a plain warm chain without cold
results - with the condition under which the GPU tests may ask for bit equality of decisions taken in float32: on every case they
use, every frame's float64 warm / cold rms ratio lies outside [recover_ratio / 1.25, recover_ratio x 1.25].  DESIGN.md, "Sequences
tracked in one launch"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import start_cases as sc
import track_cases as tk
import views_cases as vc
from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "track_c99.c"), "-o", str(tmp_path / "track_c99.o")])


def test_prototype_table_matches_the_header():
    """The ut_* declaration of umetrack_hip_track.h has one entry in the binding's table of its own with as many argtypes as the C
    declaration has parameters, load_library() declares it, and no older table names it."""
    text = open(os.path.join(ROOT, "include", "umetrack_hip_track.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_track_pose_views": 38}
    assert set(declared) == set(_native.TRACK_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS) | set(_native.VIEWS_EXPORTS) | set(_native.ROBUST_EXPORTS) | set(_native.VIEWS_SCALE_EXPORTS)
             | set(_native.UNCERTAINTY_EXPORTS) | set(_native.SMOOTH_EXPORTS) | set(_native.START_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    vp, i32, f32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_double
    restype, argtypes = _native._TRACK_PROTOTYPES["ut_track_pose_views"]
    fn = lib.ut_track_pose_views
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes) and declared["ut_track_pose_views"] == len(argtypes)
    # handle | model | window weights cam_rows max_views table n_rows kind | limits | init | cold | rule | lengths | mirror t_scale max_iters
    # loss loss_scale | n_seq n_frames | pose out | info chosen | stream
    assert list(argtypes) == [vp, vp, i32] + [vp, vp, vp, i32, vp, i32, i32] + [vp] + [vp, i32, vp, i32] + [vp, i32, vp, i32, vp, vp] + \
        [f64, f64] + [vp] + [vp, f32, i32, i32, f32] + [i32, i32] + [vp, i32, vp, i32] + [vp, vp] + [vp]
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(UT_TRACK_[A-Z_]+)\s+(\d+)\s", text)}
    assert codes == dict(UT_TRACK_WARM=0, UT_TRACK_COLD=1, UT_TRACK_NONE=2)
    assert (_native.UT_TRACK_WARM, _native.UT_TRACK_COLD, _native.UT_TRACK_NONE) == (tk.WARM, tk.COLD, tk.NONE) == (0, 1, 2)
    assert '#include "umetrack_hip_start.h"' in text


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed."""
    lib = _native.load_library()
    bufs = dict(hm=np.ones(321, np.float32), win=np.ones(6 * 2 * 42), rows=np.zeros(12, np.int32), tab=np.ones(32), ija=np.zeros(2 * 22, np.float32),
                ixf=np.zeros(2 * 16, np.float32), cja=np.zeros(6 * 22, np.float32), cxf=np.zeros(6 * 16, np.float32), cinfo=np.zeros(24, np.float32),
                cidx=np.zeros(6, np.int32), ja=np.zeros(6 * 22, np.float32), xf=np.zeros(6 * 16, np.float32), info=np.zeros(24, np.float32),
                chosen=np.zeros(6, np.int32))
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, n_models=1, max_views=2, n_rows=1, kind=0, ija_stride=22, ixf_stride=16, cja_stride=22,
                cxf_stride=16, ratio=1.5, floor=0.01, t_scale=1.0, max_iters=32, loss=0, loss_scale=3.0, n_seq=2, n_frames=3, ja_stride=22,
                xf_stride=16)

    def call(**change):
        a = dict(good, **change)
        rc = lib.ut_track_pose_views(None, a["hm"], a["n_models"], a["win"], None, a["rows"], a["max_views"], a["tab"], a["n_rows"], a["kind"], None,
                                     a["ija"], a["ija_stride"], a["ixf"], a["ixf_stride"], a["cja"], a["cja_stride"], a["cxf"], a["cxf_stride"],
                                     a["cinfo"], a["cidx"], ctypes.c_double(a["ratio"]), ctypes.c_double(a["floor"]), None, None,
                                     ctypes.c_float(a["t_scale"]), a["max_iters"], a["loss"], ctypes.c_float(a["loss_scale"]), a["n_seq"],
                                     a["n_frames"], a["ja"], a["ja_stride"], a["xf"], a["xf_stride"], a["info"], a["chosen"], None)
        return rc, lib.ut_last_error(None).decode()

    nan, inf = float("nan"), float("inf")
    no_cold = dict(cja=None, cxf=None, cinfo=None, cidx=None)
    for change, word in (
            # what ut_fit_pose_views_robust lists
            (dict(hm=None), "bad argument"), (dict(win=None), "null"), (dict(rows=None), "null"), (dict(tab=None), "null"), (dict(ja=None), "bad argument"),
            (dict(xf=None), "bad argument"), (dict(kind=2), "table_kind"), (dict(max_views=0), "max_views"), (dict(max_views=9), "max_views"),
            (dict(n_rows=0), "bad argument"), (dict(n_models=3), "bad argument"), (dict(loss=3), "loss"), (dict(loss=1, loss_scale=0.0), "loss_scale"),
            (dict(loss=2, loss_scale=nan), "loss_scale"), (dict(max_iters=0), "max_iters"), (dict(max_iters=257), "max_iters"),
            (dict(ja_stride=21), "stride"), (dict(xf_stride=11), "stride"), (dict(ija_stride=21), "stride"), (dict(ixf_stride=11), "stride"),
            (dict(t_scale=0.0), "t_scale"), (dict(t_scale=nan), "t_scale"),
            # its own
            (dict(ija=None), "init_angles and init_wrist_xf"), (dict(ixf=None), "init_angles and init_wrist_xf"),
            (dict(cja=None), "cold_"), (dict(cxf=None), "cold_"), (dict(cinfo=None), "cold_"), (dict(cidx=None), "cold_"),
            (dict(no_cold, ija=None, ixf=None), "nothing to start from"), (dict(cja_stride=21), "stride"), (dict(cxf_stride=11), "stride"),
            (dict(info=None), "null"), (dict(chosen=None), "null"), (dict(n_frames=0), "n_frames"), (dict(n_seq=-1), "n_seq"),
            (dict(n_seq=1 << 20, n_frames=1 << 12, n_models=1), "fit an int"),
            (dict(ratio=0.99), "recover_ratio"), (dict(ratio=nan), "recover_ratio"), (dict(ratio=inf), "recover_ratio"),
            (dict(floor=-1e-9), "recover_floor"), (dict(floor=nan), "recover_floor"), (dict(floor=inf), "recover_floor"),
            (dict(n_seq=0, ratio=0.5), "recover_ratio")):
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("ut_track_pose_views: ") and word in msg, (change, rc, msg)
    assert call(n_seq=0)[0] == 0                                                       # nothing to do is not an error
    assert call(n_seq=0, **no_cold)[0] == 0 and call(n_seq=0, ija=None, ixf=None)[0] == 0
    assert not any(bufs[k].any() for k in ("ja", "xf", "info", "chosen"))


# ----------------------------------------------------------------------------- the restatement
def test_restatement_is_start_cases_track_on_the_documented_loss():
    """Hand 1 of frames 200..263, two views, 0.5 px, from frame 200's label: track_sequences with one sequence, an init and the cold
    chain's results is start_cases.track bit for bit - frames 23, 28 and 31 recover - and start_cases.cold_fit is track_cases.cold_fit."""
    import smooth_cases as sm
    k = tk.case("loss64")
    seq = sm.recording(200, 263, 1, 2, 0.5)
    c = dict(seq["views_case"], limits=None)
    assert all(np.array_equal(k["c"][f], c[f]) for f in ("window", "cam_rows", "table", "weights", "mirror"))
    assert np.array_equal(k["init"][0], seq["truth_ja"][:1]) and np.array_equal(k["init"][1], seq["truth_xf"][:1])
    cold, mine = tk.restated("loss64")
    theirs_cold = sc.cold_fit(c, max_iters=32)
    assert all(np.array_equal(cold[f], theirs_cold[f]) for f in ("ja", "xf", "info", "index"))
    theirs = sc.track(c, theirs_cold, k["init"])
    assert np.flatnonzero(theirs["recovered"]).tolist() == [23, 28, 31]
    assert np.array_equal(mine["chosen"] == tk.COLD, theirs["recovered"]) and set(mine["chosen"]) == {tk.WARM, tk.COLD}
    assert all(np.array_equal(mine[f], theirs[f]) for f in ("ja", "xf", "info", "warm_rms"))


def test_restatement_without_cold_results_is_a_plain_warm_chain():
    """No cold arrays: every frame inside a length is views_cases.fit_views from the previous frame's result, sequence by sequence;
    rows at or past a length hold nothing."""
    k = tk.case("no_cold")
    c, t_n = k["c"], k["n_frames"]
    got = tk.restated("no_cold")[1]
    for s, length in enumerate(k["lengths"]):
        prev = (k["init"][0][s:s + 1], k["init"][1][s:s + 1])
        for t in range(length):
            i = slice(s * t_n + t, s * t_n + t + 1)
            w = vc.fit_views(c["hm"], c["window"][i], c["cam_rows"][i], c["table"], c["weights"][i], prev, c["mirror"][i])
            prev = (np.asarray(w[0], np.float32), np.asarray(w[1], np.float32))
            assert np.array_equal(got["ja"][i], prev[0]) and np.array_equal(got["xf"][i], prev[1]) and np.array_equal(got["info"][i], w[2].astype(np.float32))
        past = slice(s * t_n + length, (s + 1) * t_n)
        assert np.all(got["chosen"][s * t_n:s * t_n + length] == tk.WARM) and np.all(got["chosen"][past] == -1)
        assert not got["info"][past].any() and not got["ja"][past].any()


def test_rule_of_the_restatement():
    """What the header says about starts: without an init the first usable cold row starts a sequence (COLD), refused cold rows before
    it are NONE and hold the cold row; a frame without weights is refused, keeps its start and the next frame goes on from it; a wrong
    init is recovered from at frame 0."""
    cold, r = tk.restated("cold_refused_first")
    assert r["chosen"].tolist() == [tk.NONE, tk.NONE, tk.COLD, tk.WARM] and cold["index"][:2].tolist() == [-1, -1]
    assert np.array_equal(r["info"][:3], cold["info"][:3]) and np.array_equal(r["ja"][:3], cold["ja"][:3])
    cold, r = tk.restated("no_init")
    assert r["chosen"].tolist() == [tk.COLD, tk.WARM, tk.WARM, tk.WARM] * 2
    cold, r = tk.restated("blank_frame")
    assert r["chosen"].tolist() == [tk.WARM] * 6 and int(r["info"][3, 3]) == tk.REFUSED and cold["index"][3] == -1
    assert np.array_equal(r["ja"][3], r["ja"][2]) and np.array_equal(r["xf"][3], r["xf"][2]) and int(r["info"][4, 3]) & 1
    cold, r = tk.restated("wrong_init")
    assert r["chosen"].tolist() == [tk.COLD, tk.WARM, tk.WARM]


# ----------------------------------------------------------------------------- float32 takes the float64 decisions
@pytest.mark.parametrize("name", tk.GPU_CASES)
def test_ratios_stay_clear_of_the_threshold(name):
    """Every frame of every case tests/test_gpu_track.py uses: the float64 warm / cold rms ratio outside [RECOVER_RATIO / 1.25,
    RECOVER_RATIO x 1.25], wherever a warm fit was made and the cold row is usable (elsewhere no rms decides)."""
    k = tk.case(name)
    cold, r = tk.restated(name)
    if cold is None:
        assert not k["cold"] and set(r["chosen"]) <= {tk.WARM, -1}
        return
    decided = np.isfinite(r["warm_rms"]) & (cold["index"] >= 0) & ((r["info"][:, 3].astype(np.int64) & tk.REFUSED) == 0)
    ratio = r["warm_rms"][decided] / cold["info"][decided, 0].astype(np.float64)
    lo, hi = tk.RECOVER_RATIO / tk.BAND, tk.RECOVER_RATIO * tk.BAND
    print(f"{name}: {int(decided.sum())} decided frames, ratios below the band at most {ratio[ratio < lo].max(initial=0):.4f}, above it at least "
          f"{ratio[ratio > hi].min(initial=np.inf):.3f}")
    assert decided.any() and np.all((ratio < lo) | (ratio > hi)), ratio[(ratio >= lo) & (ratio <= hi)]
    assert np.array_equal(r["chosen"][decided] == tk.COLD, ratio > tk.RECOVER_RATIO)
