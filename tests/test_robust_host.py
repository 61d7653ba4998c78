"""CPU tests of the robust pose fit in the views (ut_fit_pose_views_robust, include/umetrack_hip_robust.h): the numpy restatement
of tests/robust_cases.py that the GPU tests compare with - with psi = 1 it is views_cases.fit_views bit for bit, its 63 reduced
rows give the stacked reweighted normal equations, twice its gradient is the robust cost's own against central differences - the
purpose check on contaminated detections, and the C boundary.

Measured, float64, the 74 golden hands in their two seeing views, exact windows with 2 detections per view displaced by 40 px,
tracking starts +-0.05 rad / +-5 mm, Geman-McClure at 3 px: 70 of 74 hands selected (every restatement of step_cases.RUNS converged
within 24 iterations, float64 within 0.1 mm of the truth, float32 within 1 mm); on those the squared fit's median landmark error
is 48.6 mm, the robust fit's 0.0028 mm: 1.75e4 x.  DESIGN.md, "Pose from keypoints in the views, robust"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import robust_cases as rc
import step_cases as st
import views_cases as vc
from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "robust_c99.c"), "-o", str(tmp_path / "robust_c99.o")])


def test_prototype_table_matches_the_header():
    """The ut_* declaration of umetrack_hip_robust.h has one entry in the binding's table of its own with as many argtypes as the C
    declaration has parameters, load_library() declares it, no older header or table names it, and the loss codes agree."""
    text = open(os.path.join(ROOT, "include", "umetrack_hip_robust.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_fit_pose_views_robust": 29}
    assert set(declared) == set(_native.ROBUST_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS) | set(_native.VIEWS_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._ROBUST_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the robust entry is ut_fit_pose_views' list with (loss, loss_scale) behind max_iters and inlier behind residual
    views = list(_native._VIEWS_PROTOTYPES["ut_fit_pose_views"][1])
    assert list(_native._ROBUST_PROTOTYPES["ut_fit_pose_views_robust"][1]) == \
        views[:18] + [ctypes.c_int32, ctypes.c_float] + views[18:25] + [ctypes.c_void_p] + views[25:]
    for other in ("umetrack_hip.h", "umetrack_hip_fit.h", "umetrack_hip_triangulate.h", "umetrack_hip_scale.h", "umetrack_hip_info.h",
                  "umetrack_hip_views.h"):
        assert "ut_fit_pose_views_robust" not in open(os.path.join(ROOT, "include", other)).read()
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(UT_LOSS_[A-Z_]+)\s+(\d+)", header)}
    assert codes == dict(UT_LOSS_SQUARED=0, UT_LOSS_HUBER=1, UT_LOSS_GEMAN_MCCLURE=2)
    assert (_native.UT_LOSS_SQUARED, _native.UT_LOSS_HUBER, _native.UT_LOSS_GEMAN_MCCLURE) == (0, 1, 2)
    assert [_native.LOSSES[k] for k in rc.LOSSES] == [0, 1, 2] and len(_native.LOSSES) == 3
    assert '#include "umetrack_hip_views.h"' in text


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed.
    ut_fit_pose_views' checks under the entry's own name, an unknown loss, and a scale that is not finite and > 0 with a robust
    loss; with UT_LOSS_SQUARED the scale is not read."""
    lib = _native.load_library()
    n, v = 3, 2
    hm, win, w = np.zeros(321, np.float32), np.zeros(n * v * 42), np.zeros(n * v * 21, np.float32)
    rows, table = np.zeros(n * v, np.int32), np.zeros(4 * 32)
    ja, xf, info = np.zeros(n * 22, np.float32), np.zeros(n * 16, np.float32), np.zeros(n * 4, np.float32)
    res, inl = np.zeros(n * v * 21, np.float32), np.zeros(n * v * 21, np.float32)
    ija, ixf = np.ones(n * 22, np.float32), np.ones(n * 16, np.float32)
    good = dict(hm=hm.ctypes.data, n_models=1, win=win.ctypes.data, w=w.ctypes.data, rows=rows.ctypes.data, v=v, table=table.ctypes.data,
                n_rows=4, kind=0, ija=ija.ctypes.data, ija_stride=22, ixf=ixf.ctypes.data, ixf_stride=16, t_scale=1.0, iters=32, loss=2,
                scale=3.0, n=n, ja=ja.ctypes.data, ja_stride=22, xf=xf.ctypes.data, xf_stride=16, info=info.ctypes.data,
                res=res.ctypes.data, inl=inl.ctypes.data)

    def fit(**change):
        a = dict(good, **change)
        rc_ = lib.ut_fit_pose_views_robust(None, a["hm"], a["n_models"], a["win"], a["w"], a["rows"], a["v"], a["table"], a["n_rows"],
                                           a["kind"], None, a["ija"], a["ija_stride"], a["ixf"], a["ixf_stride"], None,
                                           ctypes.c_float(a["t_scale"]), a["iters"], a["loss"], ctypes.c_float(a["scale"]), a["n"], a["ja"],
                                           a["ja_stride"], a["xf"], a["xf_stride"], a["info"], a["res"], a["inl"], None)
        return rc_, lib.ut_last_error(None).decode()

    for change in (dict(loss=3), dict(loss=-1), dict(loss=1, scale=0.0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
                   dict(scale=float("inf")), dict(loss=1, scale=float("nan")), dict(ija=None), dict(ixf=None), dict(hm=None), dict(win=None),
                   dict(rows=None), dict(table=None), dict(ja=None), dict(xf=None), dict(n=-1), dict(n_models=2), dict(v=0), dict(v=9),
                   dict(kind=2), dict(n_rows=0), dict(ja_stride=21), dict(xf_stride=11), dict(iters=0), dict(iters=257), dict(t_scale=0.0),
                   dict(n=0, loss=3), dict(n=0, scale=0.0)):
        code, msg = fit(**change)
        assert code == -1 and msg.startswith("ut_fit_pose_views_robust: "), (change, code, msg)
    assert "loss must be" in fit(loss=7)[1] and "loss_scale" in fit(scale=0.0)[1] and "no cold start" in fit(ija=None, ixf=None)[1]
    assert fit(n=0)[0] == 0 and fit(n=0, loss=1)[0] == 0                   # nothing to do is not an error
    assert fit(n=0, loss=0, scale=float("nan"))[0] == 0                    # the squared loss does not read its scale
    assert fit(n=0, inl=None, res=None, info=None)[0] == 0                 # the three outputs are optional
    assert not any(b.any() for b in (ja, xf, info, res, inl))              # nothing was written
    with pytest.raises(ValueError):
        _native.loss_code("cauchy")
    assert _native.loss_code("huber") == 1 and _native.loss_code(2) == 2


# ----------------------------------------------------------------------------- the restatement
def test_with_psi_1_the_restatement_is_views_cases():
    """The loss "squared" reproduces views_cases.fit_views exactly - pose, info and residual, in float64 and in both float32
    runs, 6 iterations from the +-0.2 rad starts - and its inlier is the mask of used observations of poses not refused."""
    for name in ("two_views", "ragged"):
        c = rc.step_case(name, "squared")
        used = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64).used
        for dt, how in st.RUNS:
            got, want = rc.restate(c, dt, 6, how), vc.restate(c, dt, 6, how)
            for k in ("ja", "xf", "info", "residual"):
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, dt, how, k)
            assert np.array_equal(got["inlier"], used.astype(np.float64))


def _state(c):
    vw = rc.views_of(c)
    ang = c["init"][0].astype(np.float64)[:, :20]
    m = fc.effective_wrist(c["init"][1], c["mirror"], c["t_scale"], np.float64)
    centroid = vc.pivot(vw, fc.forward(c["hm"], ang, m, np.float64), np.float64)[0]
    return vw, ang, m, centroid


def _stacked(vw, hm, ang, m, centroid, idx):
    """The full reweighted Gauss-Newton system in float64, 2 V 21 rows weighted by sqrt(w psi)."""
    k = len(idx)
    _c, _m, _g, _good, sq, res, jacs = vw.blocks(fc.forward(hm, ang, m, np.float64), idx)
    jl = fc.jacobian(hm, ang, m, centroid, np.float64).reshape(k, 21, 3, 26)
    rows_j, rows_r = [], []
    for v in range(vw.v_max):
        sw = np.sqrt(vw.w[idx, v] * rc.psi(vw.loss, sq[:, v], vw.loss_scale))
        rows_j.append((sw[..., None, None] * (jacs[v] @ jl)).reshape(k, 42, 26))
        rows_r.append((sw[..., None] * res[v]).reshape(k, 42))
    return np.concatenate(rows_j, 1), np.concatenate(rows_r, 1)


@pytest.mark.parametrize("loss", rc.ROBUST)
@pytest.mark.parametrize("name,dirty", [("two_views", True), ("best_view", False)])
def test_reduced_rows_give_the_stacked_reweighted_normal_equations(name, dirty, loss):
    """J^T J and J^T r of the 63 reduced rows against those of the stacked 2 V 21 rows weighted by sqrt(w psi), float64, at the
    +-0.2 rad starts of the 74 golden hands, two views with 2 displaced detections each and the best view alone (rank 2): 1e-9
    relative, as test_views_host.test_reduced_rows_give_the_stacked_normal_equations.  At those starts psi is far from 1."""
    c = rc.step_case(name, loss, rc.SCALE_PX, dirty)
    vw, ang, m, centroid = _state(c)
    idx = np.arange(len(ang))
    jr, rr = vc.reduced_system(vw, c["hm"], ang, m, centroid, idx, np.float64)
    js, rs = _stacked(vw, c["hm"], ang, m, centroid, idx)
    a_r, a_s = jr.transpose(0, 2, 1) @ jr, js.transpose(0, 2, 1) @ js
    g_r, g_s = (jr.transpose(0, 2, 1) @ rr[..., None])[..., 0], (js.transpose(0, 2, 1) @ rs[..., None])[..., 0]
    d_a = float((np.abs(a_r - a_s).max((1, 2)) / np.abs(a_s).max((1, 2))).max())
    d_g = float((np.abs(g_r - g_s).max(1) / np.abs(g_s).max(1)).max())
    weights = vw.inliers(fc.forward(c["hm"], ang, m, np.float64), idx)[vw.used]
    print(f"{name}, {loss}: normal matrix {d_a:.1e} relative, gradient {d_g:.1e}; psi at the starts median {np.median(weights):.3f} min {weights.min():.1e}")
    assert np.median(weights) < 0.9 and np.abs(g_s).max() > 1 and d_a <= 1e-9 and d_g <= 1e-9


@pytest.mark.parametrize("loss", rc.ROBUST)
def test_twice_the_gradient_is_the_robust_costs_own(loss):
    """2 J^T r of the reduced rows - 2 sum w psi J^T r - against central differences of the robust cost through fc.apply_step, all
    26 parameters: 1e-6 of the gradient's largest entry, the bound and the h = 1e-5 of
    test_views_host.test_jacobian_against_central_differences, on its 8 hands outside so3_exp_map's clamp, two views with 2
    displaced detections each.  This is what makes reweighted least squares under Levenberg-Marquardt a descent method on the
    robust cost."""
    whole = rc.step_case("two_views", loss, rc.SCALE_PX, True)
    outside = np.nonzero(np.abs(whole["init"][0][:, :20]).min(1) > st.CLAMP)[0][:8]
    assert len(outside) == 8 and set(whole["mirror"][outside]) == {0, 1}
    c = rc.subset(whole, outside)
    vw, ang, m, centroid = _state(c)
    idx = np.arange(8)
    jr, rr = vc.reduced_system(vw, c["hm"], ang, m, centroid, idx, np.float64)
    grad = 2.0 * (jr.transpose(0, 2, 1) @ rr[..., None])[..., 0]

    def cost(delta):
        ta, tm = fc.apply_step(ang, m, centroid, delta)
        return vw.cost(fc.forward(c["hm"], ta, tm, np.float64), idx, np.float64)[0]

    h, num = 1e-5, np.zeros((8, 26))
    for k in range(26):
        d = np.zeros((8, 26))
        d[:, k] = h
        num[:, k] = (cost(d) - cost(-d)) / (2 * h)
    worst = float((np.abs(num - grad).max(1) / np.abs(grad).max(1)).max())
    print(f"{loss}: 2 sum w psi J^T r vs central differences of the robust cost {worst:.1e} relative")
    assert np.abs(grad).max() > 1 and worst <= 1e-6


# ----------------------------------------------------------------------------- the purpose
def test_the_robust_fit_survives_what_the_squared_fit_does_not():
    """Two views, 2 detections per view displaced by 40 px, tracking starts, Geman-McClure at 3 px, the float64 restatement: at
    least 56 of the 74 hands are selected (robust_cases.selected), and on those the squared fit's median landmark error is at
    least 100 x the robust fit's; psi < 0.5 exactly at the displaced detections."""
    c = rc.tracked_case("two", "geman_mcclure")
    sel, runs, errs = rc.selected()
    square = rc.restate(rc.with_loss(c, "squared"), np.float64, 32)
    err_sq = np.linalg.norm(vc.landmarks(c, square) - c["truth"], axis=-1).max(1)
    robust, plain = float(np.median(errs[2][sel])), float(np.median(err_sq[sel]))
    print(f"{len(sel)} of 74 hands selected; on those: squared median {plain:.1f} mm worst {err_sq[sel].max():.1f}, Geman-McClure median "
          f"{robust:.2e} mm worst {errs[2][sel].max():.2e} (float32 runs worst {errs[:2, sel].max():.2e}): {plain / robust:.1e} x; all 74: "
          f"converged {[int((r['info'][:, 3] == vc.CONVERGED).sum()) for r in runs]}, float64 worst {errs[2].max():.1f} mm")
    assert len(sel) >= 56
    assert plain >= 100.0 * robust
    used = rc.views_of(c).used
    assert np.array_equal((runs[2]["inlier"] < 0.5)[sel] & used[sel], c["displaced"][sel]) and c["displaced"].sum() == 74 * 2 * 2
