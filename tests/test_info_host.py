"""CPU tests of keypoints with their information (ut_triangulate_points_info / ut_fit_pose_info, include/umetrack_hip_info.h): the
numpy restatement of tests/info_cases.py that the GPU tests compare with - the factor against the normal equations and sigma,
the isotropic special case against fc.fit, the gain in accuracy and the calibration of the factor on noisy windows, the
decisions - and the C boundary.

The noisy runs are the golden case of tests/triangulate_cases.py (74 hands x 21 landmarks, the reference's windows, two used
views each) with default_rng(seed).normal(0, noise) on the whole window array, through info_cases.chain: triangulation with
factor -> isotropic fit (weights 1 / 0, cold) -> information fit started from it.  Measured, float64 (float32 agrees to the
digits shown), rms landmark error in mm pooled over the 74 x 21 landmarks against the reference's landmarks:

    noise px, seed   triangulated   isotropic   information   ratio   cost / 37 / noise^2   at max_iters f64 / f32
    0.25, 0              2.62         1.571        0.751       0.48        0.971                  0 / 1
    0.25, 1              2.61         1.490        0.699       0.47        0.978                  0 / 0
    0.25, 2              2.79         1.644        0.736       0.45        1.041                  0 / 1
    1,    0             10.48         6.848        3.209       0.47        0.967                  2 / 2
    1,    1             10.53         6.811        4.297       0.63        0.997                  0 / 1
    1,    2             11.23         7.362        3.644       0.50        1.072                  2 / 2

The stop rule is fc.fit's, unchanged: the poses that run to max_iters = 32 sit in the valley along depth, where accepted steps
keep lowering the cost by more than DECREASE_TOL of very little."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import info_cases as ic
import mesh_cases as mc
import triangulate_cases as tc
from absolutetrack_amd import _native, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISY = [(0.25, 0), (0.25, 1), (0.25, 2), (1.0, 0), (1.0, 1), (1.0, 2)]


@pytest.fixture(scope="module")
def golden():
    g = ic.golden_hands()
    g["tri"] = ic.triangulate_info(g["window"], g["cam_rows"], g["table"], g["weights"])
    return g


@pytest.fixture(scope="module")
def noisy(golden):
    """(noise, seed) -> {float64: chain, float32: chain}, computed once."""
    return {key: {dt: ic.chain(golden, ic.noisy_windows(golden, *key), dtype=dt) for dt in (np.float64, np.float32)} for key in NOISY}


def _pooled_rms(p, truth):
    return float(np.sqrt((np.linalg.norm(p - truth, axis=-1) ** 2).mean()))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entries_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "info_c99.c"), "-o", str(tmp_path / "info_c99.o")])


def test_prototype_table_matches_the_header():
    """Every ut_* declaration of umetrack_hip_info.h has one entry in the binding's table of its own with as many argtypes as
    the C declaration has parameters, load_library() declares it, no older header names it and the older tables are what
    they were."""
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "umetrack_hip_info.h")).read(), flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_triangulate_points_info": 18, "ut_fit_pose_info": 21}
    assert set(declared) == set(_native.INFO_EXPORTS)
    older = set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
    assert not set(declared) & older
    assert _native.EXTENSION_EXPORTS == ("ut_fit_pose",) and _native.TRIANGULATE_EXPORTS == ("ut_triangulate_points",)
    assert _native.SCALE_EXPORTS == ("ut_fit_pose_scale", "ut_pool_scale")
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._INFO_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the entries are their older twins plus one pointer / with a pointer in the same place
    tri, fit = _native._TRIANGULATE_PROTOTYPES["ut_triangulate_points"][1], _native._EXTENSION_PROTOTYPES["ut_fit_pose"][1]
    assert _native._INFO_PROTOTYPES["ut_triangulate_points_info"][1] == tri[:-1] + [ctypes.c_void_p, tri[-1]]
    assert _native._INFO_PROTOTYPES["ut_fit_pose_info"][1] == fit
    for other in ("umetrack_hip.h", "umetrack_hip_fit.h", "umetrack_hip_triangulate.h", "umetrack_hip_scale.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "ut_triangulate_points_info" not in text and "ut_fit_pose_info" not in text
    assert re.search(r"#define UT_INFO_FACTOR_FLOATS\s+6\b", header)
    assert (ic.CONVERGED, ic.AT_MAX_ITERS, ic.REFUSED) == (_native.UT_FIT_CONVERGED, _native.UT_FIT_AT_MAX_ITERS, _native.UT_FIT_REFUSED)


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed."""
    lib = _native.load_library()
    n, v, p = 3, 2, 5
    win, w = np.zeros(n * v * p * 2), np.zeros(n * v * p, np.float32)
    rows, table = np.zeros(n * v, np.int32), np.zeros(4 * 32)
    pts, pts32, info, res = np.zeros(n * p * 3), np.zeros(n * 20, np.float32), np.zeros(n * p * 4, np.float32), np.zeros(n * v * p, np.float32)
    fac = np.zeros(n * p * 6, np.float32)
    good = dict(win=win.ctypes.data, w=w.ctypes.data, rows=rows.ctypes.data, v=v, table=table.ctypes.data, n_rows=4, kind=0, p=p, n=n,
                iters=16, pts=pts.ctypes.data, pts32=pts32.ctypes.data, stride=20, info=info.ctypes.data, res=res.ctypes.data,
                fac=fac.ctypes.data)

    def tri(**change):
        a = dict(good, **change)
        rc = lib.ut_triangulate_points_info(None, a["win"], a["w"], a["rows"], a["v"], a["table"], a["n_rows"], a["kind"], a["p"],
                                            a["n"], a["iters"], a["pts"], a["pts32"], a["stride"], a["info"], a["res"], a["fac"], None)
        return rc, lib.ut_last_error(None).decode()

    for change in (dict(fac=None), dict(win=None), dict(rows=None), dict(table=None), dict(pts=None, pts32=None), dict(stride=14),
                   dict(v=0), dict(v=9), dict(iters=0), dict(iters=65), dict(p=0), dict(n=-1), dict(kind=2), dict(kind=-1), dict(n_rows=0)):
        rc, msg = tri(**change)
        assert rc == -1 and msg.startswith("ut_triangulate_points_info: "), (change, rc, msg)
    assert tri(n=0)[0] == 0                                                # nothing to do is not an error
    assert tri(n=0, fac=None)[0] == -1 and tri(n=0, win=None)[0] == -1      # but a null argument still is
    assert not any(b.any() for b in (pts, pts32, info, res, fac))           # nothing was written

    hm, tg, f = np.zeros(321, np.float32), np.zeros(n * 63, np.float32), np.zeros(n * 21 * 6, np.float32)
    ja, xf, fit_info = np.zeros(n * 22, np.float32), np.zeros(n * 16, np.float32), np.zeros(n * 4, np.float32)
    good = dict(hm=hm.ctypes.data, n_models=1, tg=tg.ctypes.data, t_stride=63, f=f.ctypes.data, ija=None, ija_stride=22, ixf=None,
                ixf_stride=16, t_scale=1.0, iters=32, n=n, ja=ja.ctypes.data, ja_stride=22, xf=xf.ctypes.data, xf_stride=16,
                info=fit_info.ctypes.data)

    def fit(**change):
        a = dict(good, **change)
        rc = lib.ut_fit_pose_info(None, a["hm"], a["n_models"], a["tg"], a["t_stride"], a["f"], None, a["ija"], a["ija_stride"], a["ixf"],
                                  a["ixf_stride"], None, ctypes.c_float(a["t_scale"]), a["iters"], a["n"], a["ja"], a["ja_stride"], a["xf"],
                                  a["xf_stride"], a["info"], None)
        return rc, lib.ut_last_error(None).decode()

    for change in (dict(f=None), dict(hm=None), dict(tg=None), dict(ja=None), dict(xf=None), dict(n=-1), dict(n_models=2),
                   dict(ija=ja.ctypes.data), dict(ixf=xf.ctypes.data), dict(t_stride=62), dict(ja_stride=21), dict(xf_stride=11),
                   dict(ija=ja.ctypes.data, ixf=xf.ctypes.data, ija_stride=21), dict(ija=ja.ctypes.data, ixf=xf.ctypes.data, ixf_stride=11),
                   dict(iters=0), dict(iters=257), dict(t_scale=0.0), dict(t_scale=float("nan")), dict(t_scale=float("inf"))):
        rc, msg = fit(**change)
        assert rc == -1 and msg.startswith("ut_fit_pose_info: "), (change, rc, msg)
    assert fit(n=0)[0] == 0
    assert not any(b.any() for b in (ja, xf, fit_info))
    # the older entries answer under their own names
    assert lib.ut_fit_pose(None, None, 1, None, 63, None, None, None, 22, None, 16, None, ctypes.c_float(1.0), 32, 1, None, 22, None, 16,
                           None, None) == -1 and lib.ut_last_error(None).decode() == "ut_fit_pose: bad argument"
    assert lib.ut_triangulate_points(None, None, None, None, 2, None, 4, 0, 5, 3, 16, None, None, 0, None, None, None) == -1
    assert lib.ut_last_error(None).decode() == "ut_triangulate_points: null argument"


# ----------------------------------------------------------------------------- the factor
def test_factor_is_the_cholesky_factor_of_the_normal_equations(golden):
    """L L^T equals the H of tc._normal_equations at the returned point to 1e-12 relative (of H's largest entry), and
    sqrt(trace((L L^T)^-1)) equals tc.triangulate's sigma to float32 rounding (2^-23 relative: sigma is that float64 number
    rounded once)."""
    g = golden
    pts, info, _res, _it, fac = g["tri"]
    assert fac.shape == (74, 21, 6) and np.all(info[..., 3] == tc.CONVERGED) and np.all((fac != 0).any(-1))
    n, v_max, n_pts = g["window"].shape[:3]
    big = n * n_pts
    rows = np.repeat(g["cam_rows"][:, None, :], n_pts, 1).reshape(big, v_max)
    w = g["weights"].astype(np.float64).transpose(0, 2, 1).reshape(big, v_max)
    win = g["window"].transpose(0, 2, 1, 3).reshape(big, v_max, 2)
    _c, h, _g, _good, _d = tc._normal_equations(g["table"][rows], win, w, w > 0, pts.reshape(big, 3), tc.FISHEYE62)
    hm = np.zeros((big, 3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        hm[:, i, j] = hm[:, j, i] = h[k]
    l = ic.matrix(fac.reshape(big, 6))
    llt = l @ l.transpose(0, 2, 1)
    rel = float((np.abs(llt - hm).max((1, 2)) / np.abs(hm).max((1, 2))).max())
    sigma = np.sqrt(np.trace(np.linalg.inv(llt), axis1=1, axis2=2))
    d_sigma = float(np.abs(sigma / info.reshape(big, 4)[:, 1].astype(np.float64) - 1).max())
    ratio = float((np.linalg.eigvalsh(hm)[:, 2] / np.linalg.eigvalsh(hm)[:, 0]).max())
    print(f"L L^T vs H: {rel:.2e} relative; sigma from the factor vs tc.triangulate's: {d_sigma:.2e} relative; largest / smallest "
          f"eigenvalue of H up to {ratio:.0f}")
    assert rel <= 1e-12 and d_sigma <= 2.0 ** -23
    assert np.all(l[:, 0, 0] > 0) and np.all(l[:, 1, 1] > 0) and np.all(l[:, 2, 2] > 0)


def test_factor_is_zero_where_the_point_is_not_known():
    for name, c in tc.decision_cases().items():
        _pts, info, _res, _it, fac = ic.triangulate_info(c["window"], c["cam_rows"], c["table"], c["weights"])
        dead = (info[..., 3].astype(int) & (tc.REFUSED | tc.DEGENERATE)) != 0
        assert np.all(fac[dead] == 0) and np.all((fac[~dead] != 0).any(-1)) and np.all(np.isinf(info[dead][:, 1])), name
        if name in ("one_view", "same_camera_twice"):
            assert dead.all(), name
        if name in ("negative_weight", "nan_at_weight_1"):
            assert dead.sum() == 1, name


# ----------------------------------------------------------------------------- the fit
@pytest.fixture(scope="module")
def rec00():
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand = mc.label_poses(lab)
    sel = np.arange(0, 738, 37)[:20]
    assert set(hand[sel]) == {0, 1}
    m = fc.effective_wrist(xf[sel], hand[sel], 1.0, np.float64)
    return dict(hm=hm, ja=ja[sel], xf=xf[sel], hand=hand[sel], targets=fc.forward(hm, ja[sel, :20], m))


def test_isotropic_factors_give_the_isotropic_fit(rec00):
    """Factors sqrt(w) I: the cost, the scalar weights (3 w: the same centroid) and every decision are fc.fit's, so the poses
    are - float64, 20 label poses, both hands, cold, weights in [0.25, 4] with three landmarks switched off: landmarks to 1e-9 mm."""
    r = rec00
    rng = np.random.default_rng(3)
    w = rng.uniform(0.25, 4.0, (20, 21))
    w[:, [2, 9, 17]] = 0
    tg = r["targets"].copy()
    tg[:, 9] = np.nan
    want = fc.fit(r["hm"], tg, weights=w, mirror=r["hand"])
    got = ic.fit_info(r["hm"], tg, ic.isotropic(w), mirror=r["hand"])
    m = lambda o: fc.forward(r["hm"], o[0][:, :20], fc.effective_wrist(o[1], r["hand"], 1.0, np.float64))
    d = float(np.linalg.norm(m(got) - m(want), axis=-1).max())
    print(f"sqrt(w) I vs fc.fit: {d:.2e} mm, iterations {got[2][:, 2].astype(int)} vs {want[2][:, 2].astype(int)}")
    assert d <= 1e-9 and np.array_equal(got[2][:, 2:], want[2][:, 2:])
    # whitened rms = sqrt(sum w d^2 / (3 used)), Euclidean worst as fc.fit's
    assert np.allclose(got[2][:, 0], want[2][:, 0] * np.sqrt(w.sum(1) / (3 * 18)), rtol=1e-6, atol=1e-12) and np.allclose(got[2][:, 1], want[2][:, 1], atol=1e-9)


def test_exact_windows_reach_the_hand(golden):
    """Exact windows, warm from the isotropic fit.  The 74 hands of the golden case as the model poses them in float64 (the
    label poses through fc.forward) seen through the golden cameras: float64 <= 1e-5 mm on every landmark, float32 printed
    beside it.  The reference's own windows are the projections of its float32 landmarks (triangulating them gives those back
    to 2e-12 mm), which lie up to 6.8e-5 mm off anything the model can pose - the isotropic float64 fit stays 3.5e-5 mm
    from them - so on those the figure is printed and held to the project's keypoint tolerance, 1e-3 mm.
    Measured: posed hands float64 8.4e-6 mm in 3 iterations, float32 7.3e-5 mm; the reference's windows float64 9.1e-5 mm, float32 9.4e-5 mm,
    2.5e-6 rad between the two."""
    g = golden
    lab = pipeline.load_labels()
    z = np.load(os.path.join(tc.GOLDEN, "projection_rec00.npz"))
    ja, xf, hand = mc.label_poses(lab)
    sel = 2 * z["frame"][z["case_frame"]] + z["hand"]
    assert np.array_equal(hand[sel], g["hand"])
    posed = fc.forward(g["hm"], ja[sel, :20], fc.effective_wrist(xf[sel], hand[sel], 1.0, np.float64))
    off = float(np.linalg.norm(posed - g["landmarks"], axis=-1).max())
    tab = g["table"][g["cam_rows"]]                                        # [74,4,32]
    win = np.stack([tc.project(tab[:, v, None, :], posed, tc.FISHEYE62)[0] for v in range(4)], 1)
    assert np.abs(win - g["window"])[g["weights"] > 0].max() < 1e-3        # the same hands to 1e-3 px
    # the float64 chain on float64 points: nothing is rounded to float32 on the way
    pts, _tri, _res, _it, fac = ic.triangulate_info(win, g["cam_rows"], g["table"], g["weights"])
    iso = fc.fit(g["hm"], pts, mirror=g["hand"])
    got = ic.fit_info(g["hm"], pts, fac, init=iso[:2], mirror=g["hand"])
    d64 = float(np.linalg.norm(ic.landmarks_of(g, got[0], got[1]) - posed, axis=-1).max())
    c32 = ic.chain(g, win, dtype=np.float32)
    d32 = float(np.linalg.norm(ic.landmarks_of(g, *c32["info"][:2]) - posed, axis=-1).max())
    print(f"posed hands (up to {off:.1e} mm from the reference's float32 landmarks): float64 {d64:.2e} mm in {int(got[2][:, 2].max())} "
          f"iterations, float32 {d32:.2e} mm in {int(c32['info'][2][:, 2].max())}")
    assert np.all(got[2][:, 3] == ic.CONVERGED) and np.all(c32["info"][2][:, 3] == ic.CONVERGED)
    assert d64 <= 1e-5
    ref = {dt: ic.chain(g, g["window"], dtype=dt) for dt in (np.float64, np.float32)}
    r64, r32 = (float(np.linalg.norm(ic.landmarks_of(g, *ref[dt]["info"][:2]) - g["landmarks"], axis=-1).max()) for dt in (np.float64, np.float32))
    ang = float(fc.angle_distance(ref[np.float32]["info"][0][:, :20], ref[np.float64]["info"][0][:, :20]).max())
    print(f"the reference's windows: float64 {r64:.2e} mm, float32 {r32:.2e} mm, {ang:.2e} rad apart, at most "
          f"{int(ref[np.float32]['info'][2][:, 2].max())} iterations")
    assert r64 <= 1e-3 and r32 <= 1e-3 and np.all(ref[np.float32]["info"][2][:, 3] == ic.CONVERGED)


def test_information_halves_the_error_on_noisy_windows(golden, noisy):
    """Noise 0.25 px and 1 px, seeds 0, 1, 2, all 74 hands: the pooled rms landmark error of the information fit is at most
    0.75 x the isotropic fit's, in both precisions (module docstring: 0.45 - 0.63)."""
    truth = golden["landmarks"].astype(np.float64)
    for key in NOISY:
        for dt in (np.float64, np.float32):
            c = noisy[key][dt]
            iso, inf = ic.landmarks_of(golden, *c["iso"][:2]), ic.landmarks_of(golden, *c["info"][:2])
            e_iso, e_inf = _pooled_rms(iso, truth), _pooled_rms(inf, truth)
            per_hand = np.sqrt((np.linalg.norm(inf - truth, axis=-1) ** 2).mean(1)) < np.sqrt((np.linalg.norm(iso - truth, axis=-1) ** 2).mean(1))
            at_max = int(((c["info"][2][:, 3].astype(int) & ic.AT_MAX_ITERS) != 0).sum())
            print(f"{key[0]} px, seed {key[1]}, {dt.__name__}: triangulated {_pooled_rms(c['points'], truth):.2f} mm, isotropic {e_iso:.3f}, "
                  f"information {e_inf:.3f}, ratio {e_inf / e_iso:.2f}; better on {100 * per_hand.mean():.0f} % of the hands; {at_max} of 74 at "
                  f"max_iters = 32, iterations mean {c['info'][2][:, 2].mean():.1f}")
            assert c["info"][0].dtype == dt and not np.any(c["info"][2][:, 3].astype(int) & ic.REFUSED)
            assert e_inf <= 0.75 * e_iso


def test_the_factor_is_calibrated(noisy):
    """cost / (63 - 26) / noise^2, averaged over the 74 hands, lies in [0.85, 1.15]: the whitened residuals are the views'
    reprojection residuals to first order, a chi^2 with the 26 fitted parameters taken out (4 x 21 window coordinates less 3 x
    21 point coordinates leave 21 per hand that the triangulation keeps to itself).  A transposed factor or H in place of L
    fails this (module docstring: 0.97 - 1.07)."""
    for key in NOISY:
        for dt in (np.float64, np.float32):
            info = noisy[key][dt]["info"][2].astype(np.float64)
            chi = float((info[:, 0] ** 2 * 63 / (63 - 26) / key[0] ** 2).mean())
            print(f"{key[0]} px, seed {key[1]}, {dt.__name__}: cost / 37 / noise^2 = {chi:.3f}")
            assert 0.85 <= chi <= 1.15


def test_decisions(rec00):
    r = rec00
    n = 6
    tg = r["targets"][:n].copy()
    rng = np.random.default_rng(5)
    f = ic.matrix(np.zeros((n, 21, 6)))
    f[..., 0, 0], f[..., 1, 1], f[..., 2, 2] = rng.uniform(0.5, 2, (3, n, 21))
    f[..., 1, 0], f[..., 2, 0], f[..., 2, 1] = rng.uniform(-0.5, 0.5, (3, n, 21))
    f = np.stack([f[..., 0, 0], f[..., 1, 0], f[..., 1, 1], f[..., 2, 0], f[..., 2, 1], f[..., 2, 2]], -1)
    clean = ic.fit_info(r["hm"], tg, f, init=(r["ja"][:n], r["xf"][:n]), mirror=r["hand"][:n])
    assert np.all(clean[2][:, 3] == ic.CONVERGED) and np.linalg.norm(ic_landmarks(r, clean, n) - tg, axis=-1).max() <= 1e-5
    f2, tg2 = f.copy(), tg.copy()
    f2[0, 4] = 0
    tg2[0, 4] = np.nan                            # a zero factor with a NaN target changes nothing ...
    f3, tg3 = f2.copy(), tg.copy()
    tg3[0, 4] = 123.5                             # ... against finite garbage there
    f2[1, 7, 3] = np.nan                          # a NaN factor entry refuses
    f2[2] = 0
    f2[2, [0, 5], 0] = 1.0                        # two used landmarks refuse
    tg2[3, 2, 1] = np.inf                         # a non-finite target of a used landmark refuses
    f2[4, 6, 4] = 0.25                            # an off-diagonal entry alone makes a landmark used
    f2[4, 6, [0, 1, 2, 3, 5]] = 0
    init = (r["ja"][:n] + 0.01, r["xf"][:n])
    got = ic.fit_info(r["hm"], tg2, f2, init=init, mirror=r["hand"][:n])
    ref = ic.fit_info(r["hm"], tg3, f3, init=init, mirror=r["hand"][:n])
    assert np.array_equal(got[2][:, 3], [1, 4, 4, 4, 1, 1]) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(got, ref)) and all(np.array_equal(a[5], b[5]) for a, b in zip(got, ref))
    assert np.array_equal(got[0][1:4], init[0][1:4]) and np.array_equal(got[1][1:4], init[1][1:4]) and not got[2][1:4, :3].any()
    cold = ic.fit_info(r["hm"], tg2, f2, mirror=r["hand"][:n])
    assert np.array_equal(cold[2][:, 3] == ic.REFUSED, [False, True, True, True, False, False]) and not cold[0][1:4].any()
    assert np.array_equal(cold[1][1:4], np.tile(np.eye(4), (3, 1, 1)))


def ic_landmarks(r, out, n):
    return fc.forward(r["hm"], out[0][:, :20], fc.effective_wrist(out[1], r["hand"][:n], 1.0, np.float64))
