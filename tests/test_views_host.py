"""CPU tests of the pose fit on 2-D keypoints in camera views (ut_fit_pose_views, include/umetrack_hip_views.h): the numpy
restatement of tests/views_cases.py that the GPU tests compare with - its reduction of the stacked reprojection system to 63
rows, its Jacobian against central differences, full float64 fits on exact windows with two views and with one, the cost's
monotony, the decisions - and the C boundary.

Measured, float64, the 74 golden hands (tests/info_cases.py golden_hands), the reference's own windows, starts +-0.4 rad /
+-30 mm: two views 74 of 74 converged, worst landmark 8.9e-5 mm, at most 7 iterations; the best view alone 74 of 74, worst
landmark 1.8e-4 mm, after 2 of the 74 hands drew their start again (views_cases.full_case: the first draw lies in the basin of a
mirror pose).  Reduced rows against the stacked system at the +-0.2 rad starts: 1.2e-15 relative (normal matrix) and 4.9e-16
(gradient) with two views, 7.6e-11 and 1.3e-10 with one.  1 px noise, the second view missing 12 random landmarks: pooled rms
landmark error 28.3 mm for the chain on the landmarks both views keep, 14.7 mm refined in the views."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import step_cases as st
import triangulate_cases as tc
import views_cases as vc
from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "views_c99.c"), "-o", str(tmp_path / "views_c99.o")])


def test_prototype_table_matches_the_header():
    """Every ut_* declaration of umetrack_hip_views.h has one entry in the binding's table of its own with as many argtypes as
    the C declaration has parameters, load_library() declares it, and no older header or table names it."""
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "umetrack_hip_views.h")).read(), flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_fit_pose_views": 26}
    assert set(declared) == set(_native.VIEWS_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._VIEWS_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    for other in ("umetrack_hip.h", "umetrack_hip_fit.h", "umetrack_hip_triangulate.h", "umetrack_hip_scale.h", "umetrack_hip_info.h"):
        assert "ut_fit_pose_views" not in open(os.path.join(ROOT, "include", other)).read()
    assert (vc.CONVERGED, vc.AT_MAX_ITERS, vc.REFUSED) == (_native.UT_FIT_CONVERGED, _native.UT_FIT_AT_MAX_ITERS, _native.UT_FIT_REFUSED)
    assert tc.MAX_VIEWS == _native.TRI_MAX_VIEWS


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed.  The union of
    ut_fit_pose's and ut_triangulate_points's checks, and the start is required."""
    lib = _native.load_library()
    n, v = 3, 2
    hm, win, w = np.zeros(321, np.float32), np.zeros(n * v * 42), np.zeros(n * v * 21, np.float32)
    rows, table = np.zeros(n * v, np.int32), np.zeros(4 * 32)
    ja, xf, info, res = np.zeros(n * 22, np.float32), np.zeros(n * 16, np.float32), np.zeros(n * 4, np.float32), np.zeros(n * v * 21, np.float32)
    ija, ixf = np.ones(n * 22, np.float32), np.ones(n * 16, np.float32)
    good = dict(hm=hm.ctypes.data, n_models=1, win=win.ctypes.data, w=w.ctypes.data, rows=rows.ctypes.data, v=v, table=table.ctypes.data,
                n_rows=4, kind=0, ija=ija.ctypes.data, ija_stride=22, ixf=ixf.ctypes.data, ixf_stride=16, t_scale=1.0, iters=32, n=n,
                ja=ja.ctypes.data, ja_stride=22, xf=xf.ctypes.data, xf_stride=16, info=info.ctypes.data, res=res.ctypes.data)

    def fit(**change):
        a = dict(good, **change)
        rc = lib.ut_fit_pose_views(None, a["hm"], a["n_models"], a["win"], a["w"], a["rows"], a["v"], a["table"], a["n_rows"], a["kind"],
                                   None, a["ija"], a["ija_stride"], a["ixf"], a["ixf_stride"], None, ctypes.c_float(a["t_scale"]),
                                   a["iters"], a["n"], a["ja"], a["ja_stride"], a["xf"], a["xf_stride"], a["info"], a["res"], None)
        return rc, lib.ut_last_error(None).decode()

    for change in (dict(ija=None), dict(ixf=None), dict(ija=None, ixf=None), dict(hm=None), dict(win=None), dict(rows=None),
                   dict(table=None), dict(ja=None), dict(xf=None), dict(n=-1), dict(n_models=2), dict(v=0), dict(v=9), dict(kind=2),
                   dict(kind=-1), dict(n_rows=0), dict(ja_stride=21), dict(xf_stride=11), dict(ija_stride=21), dict(ixf_stride=11),
                   dict(iters=0), dict(iters=257), dict(t_scale=0.0), dict(t_scale=float("nan")), dict(t_scale=float("inf"))):
        rc, msg = fit(**change)
        assert rc == -1 and msg.startswith("ut_fit_pose_views: "), (change, rc, msg)
    assert "no cold start" in fit(ija=None, ixf=None)[1]
    assert fit(n=0)[0] == 0                                                # nothing to do is not an error
    assert fit(n=0, ija=None)[0] == -1 and fit(n=0, win=None)[0] == -1      # but a null argument still is
    assert not any(b.any() for b in (ja, xf, info, res))                    # nothing was written
    # the older entries answer under their own names
    assert lib.ut_fit_pose(None, None, 1, None, 63, None, None, None, 22, None, 16, None, ctypes.c_float(1.0), 32, 1, None, 22, None, 16,
                           None, None) == -1 and lib.ut_last_error(None).decode() == "ut_fit_pose: bad argument"


# ----------------------------------------------------------------------------- the reduction
def _state(c, dtype=np.float64):
    """The start of a case as the solver holds it: (Views, angles, effective wrist, centroid)."""
    vw = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], dtype)
    ang = c["init"][0].astype(dtype)[:, :20]
    m = fc.effective_wrist(c["init"][1], c["mirror"], c["t_scale"], dtype)
    centroid = vc.pivot(vw, fc.forward(c["hm"], ang, m, dtype), dtype)[0]
    return vw, ang, m, centroid


@pytest.mark.parametrize("name,measured", [("two_views", 1.2e-15), ("best_view", 1.3e-10)])
def test_reduced_rows_give_the_stacked_normal_equations(name, measured):
    """J^T J and J^T r of the 63 reduced rows against those of the stacked 2 V 21 rows, float64, at the +-0.2 rad starts of the
    74 golden hands: 1e-9 relative (of the largest entry of each pose's matrix / gradient).  One view is the rank-2 case: the
    semidefinite factor drops the direction along the ray."""
    c = vc.case(name)
    vw, ang, m, centroid = _state(c)
    idx = np.arange(len(ang))
    jr, rr = vc.reduced_system(vw, c["hm"], ang, m, centroid, idx, np.float64)
    js, rs = vc.stacked_system(vw, c["hm"], ang, m, centroid, idx)
    a_r, a_s = jr.transpose(0, 2, 1) @ jr, js.transpose(0, 2, 1) @ js
    g_r, g_s = (jr.transpose(0, 2, 1) @ rr[..., None])[..., 0], (js.transpose(0, 2, 1) @ rs[..., None])[..., 0]
    d_a = float((np.abs(a_r - a_s).max((1, 2)) / np.abs(a_s).max((1, 2))).max())
    d_g = float((np.abs(g_r - g_s).max(1) / np.abs(g_s).max(1)).max())
    rank = np.linalg.matrix_rank(js[0])
    print(f"{name}: normal matrix {d_a:.1e} relative, gradient {d_g:.1e} (measured {measured:.0e}); rank of the stacked J {rank}")
    assert np.abs(g_s).max() > 1 and d_a <= 1e-9 and d_g <= 1e-9


@pytest.mark.parametrize("name", ["two_views", "pinhole", "table_a"])
def test_jacobian_against_central_differences(name):
    """The stacked residual's analytic Jacobian (camera Jacobian x fc.jacobian) against central differences of the float64
    forward function through fc.apply_step, all 26 parameters: 1e-6 of the column's largest entry, the bound of
    test_fit_host.test_jacobian_matches_central_differences, with its h = 1e-5 (rounding 1e-16 x 300 px / h against columns of
    hundreds of px per rad).  On the first 8 hands whose start has no angle inside so3_exp_map's clamp (|angle| < 0.01 rad),
    where the analytic Jacobian deliberately differs."""
    whole = vc.case(name)
    outside = np.nonzero(np.abs(whole["init"][0][:, :20]).min(1) > st.CLAMP)[0][:8]
    assert len(outside) == 8 and set(whole["mirror"][outside]) == {0, 1}
    c = vc.subset(whole, outside)
    vw, ang, m, centroid = _state(c)
    idx = np.arange(len(ang))
    js, _rs = vc.stacked_system(vw, c["hm"], ang, m, centroid, idx)

    def residual(delta):
        ta, tm = fc.apply_step(ang, m, centroid, delta)
        _c, _m, _g, _good, _sq, res, _j = vw.blocks(fc.forward(c["hm"], ta, tm, np.float64), idx)
        return np.concatenate([(np.sqrt(vw.w[:, v])[..., None] * res[v]).reshape(len(idx), 42) for v in range(vw.v_max)], 1)

    h, worst = 1e-5, 0.0
    for k in range(26):
        d = np.zeros((len(idx), 26))
        d[:, k] = h
        num = (residual(d) - residual(-d)) / (2 * h)
        worst = max(worst, float((np.abs(num - js[:, :, k]).max(1) / np.abs(js[:, :, k]).max(1)).max()))
    print(f"{name}: analytic vs central differences {worst:.1e} relative")
    assert worst <= 1e-6


# ----------------------------------------------------------------------------- full fits
@pytest.mark.parametrize("views,measured", [("two", 8.9e-5), ("one", 1.8e-4)])
def test_exact_windows_reach_the_hand(views, measured):
    """Float64 full fits on the reference's own windows from +-0.4 rad / +-30 mm: all 74 converge, worst landmark <= 1e-3 mm
    against the golden landmarks.  The accepted cost never rises."""
    c = vc.full_case(views)
    trace = []
    r = vc.restate(c, np.float64, 32, trace=trace)
    err = np.linalg.norm(vc.landmarks(c, r) - c["truth"], axis=-1).max(1)
    its = r["info"][:, 2].astype(int)
    print(f"{views} view(s): {int((r['info'][:, 3] == vc.CONVERGED).sum())} of 74 converged, worst landmark {err.max():.2e} mm (measured "
          f"{measured:.1e}), iterations mean {its.mean():.1f} max {its.max()}, rms up to {r['info'][:, 0].max():.1e} px; hands that drew "
          f"their start again: {np.nonzero(c['draws'] > 1)[0].tolist()} ({int(c['draws'].max())} draws at most)")
    assert np.all(r["info"][:, 3] == vc.CONVERGED) and err.max() <= st.KP_TOL_MM
    for t in trace:
        assert np.all(t["trial_cost"][t["accept"]] < t["cost"][t["accept"]])
    assert np.all(r["residual"][c["weights"] == 0] == 0) and r["residual"].max() <= 1e-3
    if views == "two":
        assert np.all(c["draws"] == 1)


def test_refining_the_chain_lowers_the_reprojection_cost():
    """1 px noise, the second view missing 12 random landmarks: started from the chain (which sees the 9 landmarks both views
    keep), the fit in the views ends at a reprojection cost over ALL detections that is at most the start's, hand by hand, and
    the accepted cost never rises on the way.  The pooled landmark error against the truth is printed."""
    c = vc.noisy_ragged()
    vw = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64)
    start = dict(ja=c["init"][0], xf=c["init"][1])
    cost0 = vw.cost(vc.landmarks(c, start), np.arange(74), np.float64)[0]
    trace = []
    r = vc.restate(c, np.float64, 32, trace=trace)
    cost1 = vw.cost(vc.landmarks(c, r), np.arange(74), np.float64)[0]
    rms = lambda p: float(np.sqrt((np.linalg.norm(p - c["truth"], axis=-1) ** 2).mean()))
    print(f"ragged, 1 px: cost {cost0.sum():.1f} -> {cost1.sum():.1f} px^2; pooled rms landmark error chain {rms(vc.landmarks(c, start)):.2f} mm, "
          f"refined in the views {rms(vc.landmarks(c, r)):.2f} mm; {int((r['info'][:, 3].astype(int) & vc.AT_MAX_ITERS != 0).sum())} of 74 at max_iters")
    assert not np.any(r["info"][:, 3].astype(int) & vc.REFUSED)
    assert np.all(cost1 <= cost0)
    for t in trace:
        assert np.all(t["trial_cost"][t["accept"]] < t["cost"][t["accept"]])
    assert rms(vc.landmarks(c, r)) < rms(vc.landmarks(c, start))


# ----------------------------------------------------------------------------- decisions
def test_decisions():
    c = vc.subset(vc.case("two_views"), np.arange(8))
    win, w, rows = c["window"].copy(), c["weights"].copy(), c["cam_rows"].copy()
    w[0, 1, 4] = 0
    win[0, 1, 4] = np.nan                         # a NaN window at weight 0 changes nothing ...
    w[1, 0, 3] = -1.0                             # a negative weight refuses
    w[2, 1, 7] = np.nan                           # so does a NaN weight
    win[3, 0, 5, 1] = np.inf                      # and a non-finite window at a positive weight
    w[4] = 0
    w[4, 0, [2, 9]] = 1                           # two landmarks with a used observation refuse
    rows[5, 1] = -1
    w[5, 1] = np.nan                              # the weights of an unused view are not read
    got = vc.restate(dict(c, window=win, weights=w, cam_rows=rows), max_iters=32)
    win2 = win.copy()
    win2[0, 1, 4] = 123.5                         # ... against finite garbage there
    ref = vc.restate(dict(c, window=win2, weights=w, cam_rows=rows), max_iters=32)
    assert np.array_equal(got["info"][:, 3], [1, 4, 4, 4, 4, 1, 1, 1])
    for k in ("ja", "xf", "info", "residual"):
        assert np.isfinite(got[k]).all() and np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["ja"][1:5], c["init"][0][1:5].astype(np.float64)) and np.array_equal(got["xf"][1:5], c["init"][1][1:5].astype(np.float64))
    assert not got["info"][1:5, :3].any() and not got["residual"][1:5].any() and not got["residual"][5, 1].any()
    err = np.linalg.norm(vc.landmarks(c, got) - c["truth"], axis=-1).max(1)
    assert err[[0, 5, 6, 7]].max() <= st.KP_TOL_MM
    with pytest.raises(ValueError):
        vc.fit_views(c["hm"], win, rows, c["table"], w, None)
    bad = rows.copy()
    bad[6, 0] = len(c["table"])
    with pytest.raises(IndexError):
        vc.restate(dict(c, cam_rows=bad))
    # a pinhole start behind a view's near plane is refused with the rest pose at the identity, like fc.fit's non-finite start
    p = vc.subset(vc.case("pinhole"), np.arange(3))
    xf = p["init"][1].copy()
    cam = p["table"][p["cam_rows"][1, 0]]
    xf[1, :3, 3] -= (2 * (cam[4:13].reshape(3, 3)[:, 2] @ (p["truth"][1].mean(0) - cam[13:16])) * cam[4:13].reshape(3, 3)[:, 2]).astype(np.float32)
    got = vc.restate(dict(p, init=(p["init"][0], xf)), max_iters=4)
    assert np.array_equal(got["info"][:, 3].astype(int) & vc.REFUSED, [0, 4, 0])
    assert not got["ja"][1].any() and np.array_equal(got["xf"][1], np.eye(4)) and not got["info"][1, :3].any()
