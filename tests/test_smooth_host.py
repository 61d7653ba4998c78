"""CPU tests of the poses smoothed over a sequence (ut_smooth_pose_sequence, include/umetrack_hip_smooth.h): the C boundary, and the
numpy restatements of tests/smooth_cases.py that the GPU tests compare with - the recursion is the dense solve, float32 keeps the
project's bounds over eight decades of step variance with the product form of M and loses them with the subtractive one, every
term of the model matters, and on recording_00 the smoothed poses lie closer to the labels than the fits and scatter by what
param_sigma says.  DESIGN.md, "Poses smoothed over a sequence"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import smooth_cases as sm
import step_cases as st
import uncertainty_cases as uc
import views_cases as vc
from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "smooth_c99.c"), "-o", str(tmp_path / "smooth_c99.o")])


def test_prototype_table_matches_the_header():
    """The ut_* declaration of umetrack_hip_smooth.h has one entry in the binding's table of its own with as many argtypes as the C
    declaration has parameters, load_library() declares it, no older table names it, and the constants agree."""
    text = open(os.path.join(ROOT, "include", "umetrack_hip_smooth.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_smooth_pose_sequence": 23}
    assert set(declared) == set(_native.SMOOTH_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS) | set(_native.VIEWS_EXPORTS) | set(_native.ROBUST_EXPORTS) | set(_native.VIEWS_SCALE_EXPORTS)
             | set(_native.UNCERTAINTY_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    for name, (restype, argtypes) in _native._SMOOTH_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # handle | pose in with strides | info, pivot, weight, lengths, centre, step_var | n_var t_scale n_seq n_frames | workspace |
    # pose out with strides | sigma, info | stream
    assert list(_native._SMOOTH_PROTOTYPES["ut_smooth_pose_sequence"][1]) == \
        [vp, vp, i32, vp, i32] + [vp] * 6 + [i32, f32, i32, i32] + [vp] + [vp, i32, vp, i32] + [vp, vp] + [vp]
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(UT_SMOOTH_[A-Z_]+)\s+(\d+)\s", header)}
    assert codes == dict(UT_SMOOTH_OK=1, UT_SMOOTH_SINGULAR=2, UT_SMOOTH_REFUSED=4, UT_SMOOTH_GAP=8, UT_SMOOTH_WORK=408)
    assert (_native.UT_SMOOTH_OK, _native.UT_SMOOTH_SINGULAR, _native.UT_SMOOTH_REFUSED, _native.UT_SMOOTH_GAP) == (sm.OK, sm.SINGULAR, sm.REFUSED, sm.GAP)
    assert _native.UT_SMOOTH_REFUSED == _native.UT_FIT_REFUSED and _native.UT_SMOOTH_WORK == sm.WORK == 408
    assert '#include "umetrack_hip_uncertainty.h"' in text


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed."""
    lib = _native.load_library()
    n = 2 * 3
    bufs = dict(ja=np.ones(n * 22, np.float32), xf=np.ones(n * 16, np.float32), info=np.ones(n * 351, np.float32), piv=np.ones(n * 3, np.float32),
                q=np.ones(26, np.float32), ws=np.zeros(n * sm.WORK, np.float32), oja=np.zeros(n * 22, np.float32), oxf=np.zeros(n * 16, np.float32))
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, ja_stride=22, xf_stride=16, n_var=1, t_scale=1.0, n_seq=2, n_frames=3, oja_stride=22,
                oxf_stride=16)

    def call(**change):
        a = dict(good, **change)
        rc = lib.ut_smooth_pose_sequence(None, a["ja"], a["ja_stride"], a["xf"], a["xf_stride"], a["info"], a["piv"], None, None, None, a["q"],
                                         a["n_var"], ctypes.c_float(a["t_scale"]), a["n_seq"], a["n_frames"], a["ws"], a["oja"], a["oja_stride"],
                                         a["oxf"], a["oxf_stride"], None, None, None)
        return rc, lib.ut_last_error(None).decode()

    for change, word in ((dict(ja=None), "joint_angles"), (dict(xf=None), "wrist_xf"), (dict(info=None), "pose_info"), (dict(piv=None), "pivot"),
                         (dict(q=None), "step_var"), (dict(ws=None), "workspace"), (dict(oja=None), "joint_angles_out"),
                         (dict(oxf=None), "wrist_xf_out"), (dict(ja_stride=21), "stride"), (dict(xf_stride=11), "stride"),
                         (dict(oja_stride=21), "stride"), (dict(oxf_stride=11), "stride"), (dict(n_var=3), "n_var"), (dict(n_var=0), "n_var"),
                         (dict(n_frames=0), "n_frames"), (dict(n_seq=-1), "n_seq"), (dict(t_scale=0.0), "t_scale"), (dict(t_scale=-1.0), "t_scale"),
                         (dict(t_scale=float("nan")), "t_scale"), (dict(t_scale=float("inf")), "t_scale"), (dict(n_seq=0, ja=None), "joint_angles"),
                         (dict(n_seq=0, n_frames=0), "n_frames")):
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("ut_smooth_pose_sequence: ") and word in msg, (change, rc, msg)
    assert call(n_seq=0, n_var=0)[0] == 0 and call(n_seq=0, n_var=1)[0] == 0               # nothing to do is not an error
    assert not bufs["ws"].any() and not bufs["oja"].any() and not bufs["oxf"].any()        # nothing was written


def test_step_sigma_from_rates_divides_by_the_frame_rate():
    from absolutetrack_amd import hand
    s = hand.step_sigma_from_rates(0.6, 0.3, 300.0, 30.0).numpy()
    assert s.shape == (26,) and s.dtype == np.float32
    assert np.allclose(s[:20], 0.02) and np.allclose(s[20:23], 0.01) and np.allclose(s[23:], 10.0)
    with pytest.raises(ValueError):
        hand.step_sigma_from_rates(0.6, 0.3, 300.0, 0.0)


# ----------------------------------------------------------------------------- the recursion is the dense solve
def _against_dense(seq, bound=1e-10):
    p = sm.prepare(seq)
    u, c, regular = sm.dense(p)
    r = sm.recursion(p)
    assert regular and r["regular"]
    us, cs = np.abs(u).max(), np.abs(c).max()
    du, dc = np.abs(r["u"] - u).max(), np.abs(r["c"] - c).max()
    print(f"T {len(u)}: |du| {du:.2e} of {us:.2e}, |dC| {dc:.2e} of {cs:.2e}")
    assert du <= bound * max(us, 1e-300) or (us == 0 and du == 0), (du, us)
    assert dc <= bound * cs, (dc, cs)
    return u, c, p


@pytest.mark.parametrize("name", ["plain", "gaps", "rank", "centre0", "metres", "freed"])
def test_recursion_is_the_dense_solve(name):
    """Float64: the forward filter, the backward pass and the marginal covariances against the 26 T x 26 T solve and its inverse's
    diagonal blocks, to 1e-10 of the scale of u and of C - with gaps at the first, a middle and the last frame, a rank-1 frame and a
    finger that one frame alone observes."""
    _against_dense(sm.case(name))


@pytest.mark.parametrize("length", [7, 3, 2, 1])
def test_recursion_is_the_dense_solve_on_ragged_lengths(length):
    """The ragged lengths of the GPU tests; T = 1: u = 0 and param_sigma = sqrt(diag H'^-1)."""
    seq = sm.cut(sm.case("gaps"), slice(1, 1 + length))
    u, c, p = _against_dense(seq)
    if length == 1:
        assert not u.any()
        want = np.sqrt(np.diagonal(np.linalg.inv(p["hp"][0])))
        assert np.allclose(sm.smooth(seq)["sigma"][0], want, rtol=1e-9, atol=0)


def test_a_gap_is_filled_by_its_neighbours():
    """A gap's H' is 0 whatever its pose_info holds, its status carries GAP, and its sigma is larger than its neighbours'."""
    seq = sm.case("gaps")
    res = sm.smooth(seq)
    assert (res["info"][:, 3] == np.where(np.isin(np.arange(12), (0, 5, 11)), sm.OK | sm.GAP, sm.OK)).all()
    assert not res["info"][[0, 5, 11], 0].any() and (res["sigma"][5] > res["sigma"][4]).all() and (res["sigma"][5] > res["sigma"][6]).all()
    other = dict(seq, pose_info=seq["pose_info"].copy(), pivot=seq["pivot"].copy())
    other["pose_info"][5], other["pivot"][5] = np.nan, np.nan
    again = sm.smooth(other)
    assert all(np.array_equal(res[k], again[k]) for k in ("ja", "xf", "sigma", "info"))


# ----------------------------------------------------------------------------- float32 over the range of q
@pytest.fixture(scope="module")
def long_sequence():
    """Frames 200..263, hand 0, two views, 0.5 px."""
    return sm.recording(200, 263, 0, 2, 0.5)


@pytest.mark.parametrize("scale", sm.Q_SCALES)
def test_float32_keeps_the_project_bounds_with_the_product_form(long_sequence, scale):
    """The float32 restatements (st.RUNS' two solves) on 64 frames against float64: within st.ANGLE_TOL_RAD / st.KP_TOL_MM at every
    scale of q.  The subtractive M = W - W S^-1 W misses them at q x 1e-4."""
    seq = sm.scaled(long_sequence, scale)
    want = sm.smooth(seq)
    for dtype, solve in st.RUNS:
        if dtype is np.float32:
            d = sm.distance(seq, sm.smooth(seq, np.float32, solve), want)
            print(f"q x {scale:g} {solve}: ang {d['ang']:.2e} rad, kp {d['kp']:.2e} mm, sigma {d['sigma']:.2e}")
            assert d["ang"] <= st.ANGLE_TOL_RAD and d["kp"] <= st.KP_TOL_MM, (scale, solve, d)
    if scale == 1e-4:
        d = sm.distance(seq, sm.smooth(seq, np.float32, "lu", product=False), want)
        print(f"q x {scale:g} subtractive: ang {d['ang']:.2e} rad, kp {d['kp']:.2e} mm")
        assert d["ang"] > st.ANGLE_TOL_RAD or d["kp"] > st.KP_TOL_MM, d


# ----------------------------------------------------------------------------- every term matters
@pytest.mark.parametrize("name,drop", [("plain", "repivot"), ("plain", "sign"), ("gaps", "weight"), ("centre0", "repivot")])
def test_wrong_restatements_are_told_apart(name, drop):
    """A restatement without the re-pivoting (B = I), with d of the wrong sign, or deaf to frame_weight moves the float64 result by
    more than the float32 restatements' distance from it."""
    seq = sm.case(name)
    want = sm.smooth(seq)
    d32 = sm.float32_distance(seq, want)
    wrong = sm.distance(seq, dict(sm.smooth(seq, drop=(drop,)), info=want["info"]), want)
    print(f"{name} without {drop}: ang {wrong['ang']:.2e} (float32 {d32['ang']:.2e}), kp {wrong['kp']:.2e} (float32 {d32['kp']:.2e})")
    assert wrong["ang"] > 10 * d32["ang"] and wrong["kp"] > 10 * d32["kp"]


# ----------------------------------------------------------------------------- quality on recording_00
SETTINGS = ((100, 139, 2, 1.0), (100, 139, 1, 1.0), (200, 263, 2, 0.5))


def _fit_and_smoothed(seq):
    return sm.rms_to_truth(seq, dict(ja=seq["ja"], xf=seq["xf"])), sm.rms_to_truth(seq, sm.smooth(seq))


def test_smoothing_brings_the_poses_closer_to_the_labels():
    """The three settings of the issue's table, both hands (noise seed 5 + hand), step variances the labels' own mean-square step:
    the smoothed landmark rms is below the fit's for every sequence, pooled over the four two-view sequences at most 0.8 of it, and
    still below it with the step variances x 0.25 and x 4."""
    pooled = np.zeros(2)
    for first, last, views, noise in SETTINGS:
        for hand in (0, 1):
            seq = sm.recording(first, last, hand, views, noise)
            (fit, fit_max), (smo, smo_max) = _fit_and_smoothed(seq)
            print(f"frames {first}..{last}, {views} views, {noise} px, hand {hand}: rms {fit:.3f} -> {smo:.3f} mm (max {fit_max:.2f} -> {smo_max:.2f})")
            assert smo < fit, (first, views, hand, fit, smo)
            for factor in (0.25, 4.0):
                assert sm.rms_to_truth(seq, sm.smooth(sm.scaled(seq, factor)))[0] < fit, (first, views, hand, factor)
            if views == 2:
                n = len(seq["ja"])
                pooled += (n * fit * fit, n * smo * smo)
    ratio = float(np.sqrt(pooled[1] / pooled[0]))
    print(f"pooled over the four two-view sequences: {ratio:.3f}")
    assert ratio <= 0.8


def test_gaps_end_closer_to_the_labels_than_their_linearisation_points():
    """Every third frame a gap whose pose is the previous frame's fit (what a tracker holds when a fit is refused): the gap frames
    end closer to the labels than that."""
    for hand in (0, 1):
        seq = sm.recording(200, 263, hand, 2, 0.5)
        n = len(seq["ja"])
        gap = np.arange(n) % 3 == 2
        held = dict(seq, ja=seq["ja"].copy(), xf=seq["xf"].copy(), weight=np.where(gap, 0, 1).astype(np.float32))
        held["ja"][gap], held["xf"][gap] = seq["ja"][np.flatnonzero(gap) - 1], seq["xf"][np.flatnonzero(gap) - 1]
        truth = sm.landmarks(seq, dict(ja=seq["truth_ja"], xf=seq["truth_xf"]))
        err = lambda res: float(np.sqrt((np.linalg.norm(sm.landmarks(seq, res) - truth, axis=-1)[gap] ** 2).mean()))
        before, after = err(held), err(sm.smooth(held))
        print(f"hand {hand}: gap frames {before:.3f} -> {after:.3f} mm")
        assert after < before


# ----------------------------------------------------------------------------- calibration
def test_param_sigma_is_the_scatter_of_the_smoothed_poses():
    """256 random walks of 8 frames drawn from the model itself (start: label frame 200, hand 0; step sigmas 0.02 rad, 0.01 rad, 1
    mm), seen by cameras 1 and 2 of that frame with 0.5 px of noise, weights 1 / sigma^2, fitted in float64 and smoothed with the
    true step variances: for every frame and parameter the mean squared error over the predicted variance lies in 1 +- 5 sqrt(2 / N)
    = 1 +- 0.442."""
    n, frames, noise = 256, 8, 0.5
    base = sm.recording(200, 200, 0, 4, noise)
    case = base["views_case"]
    hm, table = case["hm"], case["table"]
    rng = np.random.default_rng(11)
    q = sm.step_var()
    sig = np.sqrt(q.astype(np.float64))
    centre = base["centre"].astype(np.float64)
    ja = np.zeros((frames, n, 22))
    xf = np.zeros((frames, n, 4, 4))
    ja[0], xf[0] = base["truth_ja"][0], base["truth_xf"][0]
    for t in range(1, frames):
        step = rng.normal(0.0, 1.0, (n, 26)) * sig
        ja[t] = ja[t - 1]
        ja[t, :, :20] += step[:, :20]
        for i in range(n):
            e = sm.so3_exp(step[i, 20:23])
            x = xf[t - 1, i, :3, :3] @ centre + xf[t - 1, i, :3, 3]
            xf[t, i] = xf[t - 1, i]
            xf[t, i, :3, :3] = e @ xf[t - 1, i, :3, :3]
            xf[t, i, :3, 3] = x + step[i, 23:] - xf[t, i, :3, :3] @ centre
    mirror = np.zeros(n, np.int64)
    rows = np.tile(np.array([[1, 2]], np.int32), (n, 1))
    weights = np.full((n, 2, 21), 1 / noise ** 2, np.float32)
    fits = []
    for t in range(frames):
        truth = fc.forward(hm, ja[t, :, :20], fc.effective_wrist(xf[t], mirror, 1.0, np.float64))
        window = vc.exact_windows(table, rows, truth) + rng.normal(0.0, noise, (n, 2, 21, 2))
        fj, fx, info, _res = vc.fit_views(hm, window, rows, table, weights, (ja[t].astype(np.float32), xf[t].astype(np.float32)), mirror)
        assert (info[:, 3] == 1).all()
        c = dict(hm=hm, window=window, cam_rows=rows, table=table, weights=weights, mirror=mirror, t_scale=1.0, ja=fj, xf=fx, loss="squared",
                 loss_scale=3.0, angle_sigma=None)
        unc = uc.information(c)
        fits.append((fj, fx, uc.tril(unc["pose_info"]).astype(np.float32), unc["pivot"].astype(np.float32)))
    ratio = np.zeros((frames, 26))
    alone = np.zeros((frames, 26))
    for i in range(n):
        seq = dict(ja=np.stack([f[0][i] for f in fits]), xf=np.stack([f[1][i] for f in fits]), pose_info=np.stack([f[2][i] for f in fits]),
                   pivot=np.stack([f[3][i] for f in fits]), weight=None, centre=base["centre"], step_var=q, t_scale=1.0)
        res = sm.smooth(seq)
        assert (res["info"][:, 3] == sm.OK).all()
        p = sm.prepare(seq)
        for t in range(frames):
            for got, acc, var in ((res, ratio, res["sigma"][t] ** 2), (dict(ja=seq["ja"], xf=seq["xf"]), alone, np.diagonal(np.linalg.inv(p["hp"][t])))):
                rot = np.asarray(got["xf"][t], np.float64)[:3, :3]
                err = np.concatenate([sm.wrap(ja[t, i, :20] - np.asarray(got["ja"][t], np.float64)[:20]), sm.so3_log(xf[t, i, :3, :3] @ rot.T),
                                      xf[t, i, :3, :3] @ centre + xf[t, i, :3, 3] - rot @ centre - np.asarray(got["xf"][t], np.float64)[:3, 3]])
                acc[t] += err * err / var / n
    print(f"smoothed: {ratio.min():.3f} .. {ratio.max():.3f}; the fits alone: {alone.min():.3f} .. {alone.max():.3f}")
    band = 5 * np.sqrt(2 / n)
    assert abs(band - 0.442) < 1e-3 and np.all(np.abs(ratio - 1) <= band), (ratio.min(), ratio.max())


# ----------------------------------------------------------------------------- SINGULAR and refusals
def test_an_unobserved_finger_is_singular_until_one_frame_observes_it():
    free, freed = sm.smooth(sm.case("free")), sm.smooth(sm.case("freed"))
    seq = sm.case("free")
    assert (free["info"][:, 3] == sm.SINGULAR).all() and np.isinf(free["sigma"]).all() and not free["info"][:, :2].any()
    assert np.array_equal(free["ja"], seq["ja"].astype(np.float64)) and np.array_equal(free["xf"][:, :3], seq["xf"][:, :3].astype(np.float64))
    assert free["info"][11, 2] <= uc.MIN_PIVOT
    assert (freed["info"][:, 3] == sm.OK).all() and np.isfinite(freed["sigma"]).all()
    assert (freed["sigma"][:, 4:8].min(0) == freed["sigma"][6, 4:8]).all()                 # the frame that sees the finger knows it best
    for dtype, solve in st.RUNS:
        assert (sm.smooth(seq, dtype, solve)["info"][:, 3] == sm.SINGULAR).all()


def test_refusals_give_the_inputs_back():
    b = sm.case("gaps")
    for what in ("pose", "wrist", "info", "pivot", "weight", "weight_nan", "var", "var_tiny"):
        s = sm.cut(b, slice(0, 12))
        s["step_var"] = s["step_var"].copy()
        if what == "pose":
            s["ja"][4, 21] = np.inf
        elif what == "wrist":
            s["xf"][0, 1, 3] = np.nan
        elif what == "info":
            s["pose_info"][4, 100] = np.nan
        elif what == "pivot":
            s["pivot"][7, 2] = np.inf
        elif what == "weight":
            s["weight"][2] = -1.0
        elif what == "weight_nan":
            s["weight"][5] = np.nan
        elif what == "var":
            s["step_var"][25] = 0.0
        else:
            s["step_var"][3] = 1e-39                                                       # its reciprocal is not finite in float32
        for dtype, method in ((np.float64, "dense"),) + st.RUNS:
            res = sm.smooth(s, dtype, method)
            assert (res["info"] == np.array([0, 0, 0, sm.REFUSED])).all() and not res["sigma"].any(), what
            assert np.array_equal(res["ja"], s["ja"].astype(dtype), equal_nan=True) and np.array_equal(res["xf"][:, :3], s["xf"][:, :3].astype(dtype), equal_nan=True)
