"""CPU tests of the uncertainty of a pose fitted in the views (ut_pose_information_views, include/umetrack_hip_uncertainty.h): the
numpy restatement of tests/uncertainty_cases.py that the GPU tests compare with - its H is the stacked system's, carries psi,
marks exactly the free parameters, takes the prior where it belongs, and its covariance is what a Monte-Carlo run of the float64
fit on noisy detections scatters by - and the C boundary.  DESIGN.md, "Uncertainty of a pose fitted in the views"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import robust_cases as rc
import triangulate_cases as tc
import uncertainty_cases as uc
import views_cases as vc
from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "uncertainty_c99.c"), "-o", str(tmp_path / "uncertainty_c99.o")])


def test_prototype_table_matches_the_header():
    """The ut_* declaration of umetrack_hip_uncertainty.h has one entry in the binding's table of its own with as many argtypes as
    the C declaration has parameters, load_library() declares it, no older table names it, and the constants agree."""
    text = open(os.path.join(ROOT, "include", "umetrack_hip_uncertainty.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_pose_information_views": 26}
    assert set(declared) == set(_native.UNCERTAINTY_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS) | set(_native.VIEWS_EXPORTS) | set(_native.ROBUST_EXPORTS) | set(_native.VIEWS_SCALE_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._UNCERTAINTY_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the robust fit's list up to table_kind; angle_sigma for limits; the pose for the start; no max_iters; five outputs
    robust = list(_native._ROBUST_PROTOTYPES["ut_fit_pose_views_robust"][1])
    assert list(_native._UNCERTAINTY_PROTOTYPES["ut_pose_information_views"][1]) == \
        robust[:17] + robust[18:21] + [ctypes.c_void_p] * 5 + [ctypes.c_void_p]
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(UT_COV_[A-Z_]+)\s+(\d+)\s", header)}
    assert codes == dict(UT_COV_OK=1, UT_COV_SINGULAR=2, UT_COV_REFUSED=4)
    assert (_native.UT_COV_OK, _native.UT_COV_SINGULAR, _native.UT_COV_REFUSED) == (uc.OK, uc.SINGULAR, uc.REFUSED) == (1, 2, 4)
    assert _native.UT_COV_REFUSED == _native.UT_FIT_REFUSED
    floor = re.search(r"#define\s+UT_COV_MIN_PIVOT\s+([0-9.e+-]+)f", header).group(1)
    assert float(floor) == _native.UT_COV_MIN_PIVOT == uc.MIN_PIVOT == 2.0 ** -16
    assert '#include "umetrack_hip_robust.h"' in text


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed.  The robust fit's
    checks under the entry's own name, a null pose pointer, all five outputs NULL."""
    lib = _native.load_library()
    n, v = 3, 2
    hm, win, w = np.zeros(321, np.float32), np.zeros(n * v * 42), np.zeros(n * v * 21, np.float32)
    rows, table = np.zeros(n * v, np.int32), np.zeros(4 * 32)
    ja, xf = np.ones(n * 22, np.float32), np.ones(n * 16, np.float32)
    outs = [np.zeros(n * k, np.float32) for k in (351, 3, 26, 126, 4)]
    good = dict(hm=hm.ctypes.data, n_models=1, win=win.ctypes.data, w=w.ctypes.data, rows=rows.ctypes.data, v=v, table=table.ctypes.data,
                n_rows=4, kind=0, sigma=None, ja=ja.ctypes.data, ja_stride=22, xf=xf.ctypes.data, xf_stride=16, t_scale=1.0, loss=2,
                scale=3.0, n=n, o0=outs[0].ctypes.data, o1=outs[1].ctypes.data, o2=outs[2].ctypes.data, o3=outs[3].ctypes.data,
                o4=outs[4].ctypes.data)

    def call(**change):
        a = dict(good, **change)
        code = lib.ut_pose_information_views(None, a["hm"], a["n_models"], a["win"], a["w"], a["rows"], a["v"], a["table"], a["n_rows"],
                                             a["kind"], a["sigma"], a["ja"], a["ja_stride"], a["xf"], a["xf_stride"], None,
                                             ctypes.c_float(a["t_scale"]), a["loss"], ctypes.c_float(a["scale"]), a["n"], a["o0"], a["o1"],
                                             a["o2"], a["o3"], a["o4"], None)
        return code, lib.ut_last_error(None).decode()

    none = dict(o0=None, o1=None, o2=None, o3=None, o4=None)
    for change in (dict(loss=3), dict(loss=-1), dict(loss=1, scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(ja=None),
                   dict(xf=None), dict(hm=None), dict(win=None), dict(rows=None), dict(table=None), dict(n=-1), dict(n_models=2), dict(v=0),
                   dict(v=9), dict(kind=2), dict(n_rows=0), dict(ja_stride=21), dict(xf_stride=11), dict(t_scale=0.0), none,
                   dict(none, n=0), dict(n=0, loss=3)):
        code, msg = call(**change)
        assert code == -1 and msg.startswith("ut_pose_information_views: "), (change, code, msg)
    assert "all five outputs" in call(**none)[1] and "loss must be" in call(loss=7)[1]
    assert call(n=0)[0] == 0 and call(n=0, loss=0, scale=float("nan"))[0] == 0           # nothing to do is not an error
    assert call(n=0, o0=None, o1=None, o2=None, o3=None)[0] == 0                         # one output is enough
    assert not any(b.any() for b in outs)                                                # nothing was written


# ----------------------------------------------------------------------------- the restatement
def _stacked_information(c):
    """H of the full stacked system, float64: sum over views and landmarks of w psi (J_v G_l)^T (J_v G_l), no reduction."""
    n = len(c["ja"])
    idx = np.arange(n)
    vw = rc.RobustViews(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64, c["loss"], c["loss_scale"])
    ang = np.asarray(c["ja"], np.float64)[:, :20]
    m = fc.effective_wrist(c["xf"], c["mirror"], c["t_scale"], np.float64)
    p = fc.forward(c["hm"], ang, m, np.float64)
    centroid = vc.pivot(vw, p, np.float64)[0]
    _c, _m, _g, _good, sq, _res, jacs = vw.blocks(p, idx)
    gl = fc.jacobian(c["hm"], ang, m, centroid, np.float64).reshape(n, 21, 3, 26)
    h = np.zeros((n, 26, 26))
    for v in range(vw.v_max):
        rows = jacs[v] @ gl                                                              # [n,21,2,26]
        h += np.einsum("nl,nlak,nlaj->nkj", vw.w[idx, v] * rc.psi(vw.loss, sq[:, v], vw.loss_scale), rows, rows)
    return h


def _relative(h, want):
    d = np.einsum("nii->ni", want)
    return float((np.abs(h - want) / np.sqrt(d[:, :, None] * d[:, None, :])).max())


@pytest.mark.parametrize("name,bound", [("two_views", 1e-12), ("outliers_geman_mcclure", 1e-12), ("best_view", 1e-10), ("ragged", 1e-10)])
def test_reduced_information_is_the_stacked_one(name, bound):
    """H of the 63 reduced rows against H of the stacked 2 V 21 rows, float64, the 74 golden hands at their label poses: below
    1e-12 of sqrt(H_ii H_jj) where every used landmark has two views.  A landmark that one view alone sees has a rank-2 block whose
    3 x 3 factor drops a pivot at tc.PIVOT_FRACTION = 1e-10 of the block's largest entry: there the bound is that fraction (the same
    reduction is held to 1e-9 by test_views_host.test_reduced_rows_give_the_stacked_normal_equations).  The plain and the scaled
    condition numbers are printed with it."""
    c, got = uc.case(name), uc.oracle(name)["pose_info"]
    want = _stacked_information(c)
    worst = _relative(got, want)
    d = np.einsum("nii->ni", got)
    unit = got / np.sqrt(d[:, :, None] * d[:, None, :])
    plain, scaled = np.linalg.cond(got), np.linalg.cond(unit)
    print(f"{name}: reduced vs stacked H {worst:.1e} of sqrt(H_ii H_jj); condition plain median {np.median(plain):.2e} max {plain.max():.2e}, "
          f"scaled max {scaled.max():.0f}; smallest scaled pivot {uc.oracle(name)['info'][:, 2].min():.4f}, eigenvalue {np.linalg.eigvalsh(unit)[:, 0].min():.2e}")
    assert worst < bound


def test_huber_below_its_scale_is_the_squared_information():
    """At the label poses the residuals are what rounding the pose to float32 leaves, far below any scale: Huber's psi is exactly 1
    and every output equals the squared loss's, bit for bit, in float64 and float32."""
    c = uc.case("two_views")
    for dt in (np.float64, np.float32):
        want, got = uc.information(c, dt), uc.information(dict(c, loss="huber", loss_scale=2.0), dt)
        for k in want:
            assert np.array_equal(want[k], got[k]), (dt, k)


def test_geman_mcclure_is_the_squared_information_at_reweighted_detections():
    """On the displaced detections: H under Geman-McClure equals the squared loss's H with every weight multiplied by psi at the
    pose (float32 weights: to their rounding, 2^-24 per term), and the displaced detections are the ones that psi switches off.
    The pivot is the centroid under the weights as given, not under w psi, so the reweighted H is first moved to the same pivot:
    a rotation by omega about c' is one about c and a translation by omega x (c - c')."""
    c = uc.case("outliers_geman_mcclure")
    vw = rc.views_of(c)
    m = fc.effective_wrist(c["xf"], c["mirror"], c["t_scale"], np.float64)
    psi = vw.inliers(fc.forward(c["hm"], np.asarray(c["ja"], np.float64)[:, :20], m, np.float64), np.arange(len(m)))
    assert (psi[c["displaced"]] < 1e-4).all() and (psi[vw.used & ~c["displaced"]] > 0.999).all()
    got = uc.oracle("outliers_geman_mcclure")["pose_info"]
    other = uc.information(dict(c, loss="squared", weights=(c["weights"] * psi).astype(np.float32)))
    d = other["pivot"] - uc.oracle("outliers_geman_mcclure")["pivot"]                   # c' - c
    move = np.broadcast_to(np.eye(26), (len(d), 26, 26)).copy()                          # parameters about c -> about c':
    move[:, 23, 21], move[:, 23, 22], move[:, 24, 20], move[:, 24, 22], move[:, 25, 20], move[:, 25, 21] = \
        d[:, 2], -d[:, 1], -d[:, 2], d[:, 0], d[:, 1], -d[:, 0]                          # dt' = dt - hat(d) omega
    want = move.transpose(0, 2, 1) @ other["pose_info"] @ move
    worst = _relative(got, want)
    print(f"Geman-McClure vs squared at w psi: {worst:.1e} of sqrt(H_ii H_jj)")
    assert worst <= 4 * 2.0 ** -24
    assert _relative(uc.information(c, drop=("psi",))["pose_info"], got) > 0.1          # psi matters here


def test_the_free_parameters_have_a_zero_diagonal():
    """Every landmark that moves with the index finger at weight 0: exactly the columns no used landmark depends on - the
    finger's four angles - have H_ii == 0, in float64 and float32, and the pose is UT_COV_SINGULAR with +inf where promised."""
    c = uc.case("free_finger")
    free = uc.free_columns(c)
    assert np.array_equal(free, np.broadcast_to(np.isin(np.arange(26), np.arange(4 * uc.FREE_FINGER, 4 * uc.FREE_FINGER + 4)), free.shape))
    for dt, how in ((np.float64, "lu"), (np.float32, "lu"), (np.float32, "cholesky")):
        r = uc.information(c, dt, how)
        assert np.array_equal(np.einsum("nii->ni", r["pose_info"]) == 0, free), dt
        assert np.all(r["info"][:, 3] == uc.SINGULAR) and np.all(r["info"][:, 2] == 0) and np.all(np.isinf(r["info"][:, 1]))
        assert np.all(np.isinf(r["param_sigma"])) and np.all(np.isfinite(r["pose_info"])) and np.all(r["info"][:, 0] < 1e-3)
        cov = r["landmark_cov"]
        assert np.all(np.isinf(np.einsum("nlaa->nla", cov))) and np.all(cov[..., ~np.eye(3, dtype=bool)] == 0)


def _sigma_with_prior(bare, precision):
    """sqrt(diag (H + P)^-1) from H^-1 and the prior's own perturbation, Woodbury on the columns that carry a prior:
    (H + P)^-1 = H^-1 - H^-1 U (P_a^-1 + U^T H^-1 U)^-1 U^T H^-1.  bare [n,k,k], precision [k] (0 = no prior on that column)."""
    inv = np.linalg.inv(bare)
    a = np.nonzero(precision > 0)[0]
    core = np.linalg.inv(np.diag(1 / precision[a])[None] + inv[:, a][:, :, a])
    return np.sqrt(np.einsum("nii->ni", inv - inv[:, :, a] @ core @ inv[:, a, :]))


def test_the_prior_is_the_whole_answer_where_nothing_is_observed():
    """free_finger with angle_sigma: UT_COV_OK; the sigma of the four free angles is angle_sigma within 2^-21 relative.  Every other
    parameter's sigma is held to the prior's own perturbation of the information with the free columns struck out and no prior:
    Woodbury on the 16 observed angle columns gives sqrt(diag (H + P)^-1) from H^-1 exactly, and the restatement meets it to 1e-9
    relative (two float64 inverses of a matrix conditioned 4e5) - which it misses with the prior on other columns or at another
    scale.  The issue's "moves by less than the prior's share (1 / sigma_i^2) / H_ii" is not a theorem - the wrist carries no
    prior and moves through its coupling; measured 0.152 against a largest share of 0.106 - so next to the exact form stands what
    H + P <= (1 + x) H, x = share / lambda_min of the unit-diagonal matrix, gives: sigma / sqrt(1 + x) <= sigma' <= sigma."""
    c, r = uc.case("free_finger_prior"), uc.oracle("free_finger_prior")
    free = uc.free_columns(c)[0]
    sigma = np.asarray(c["angle_sigma"], np.float64)
    assert np.all(r["info"][:, 3] == uc.OK)
    at_free = np.abs(r["param_sigma"][:, free] / sigma[free[:20]] - 1).max()
    bare = uc.oracle("free_finger")["pose_info"][:, ~free][:, :, ~free]
    plain = np.sqrt(np.einsum("nii->ni", np.linalg.inv(bare)))
    got = r["param_sigma"][:, ~free]
    moved = 1 - got / plain
    precision = np.concatenate([1 / sigma ** 2, np.zeros(6)])
    exact = np.abs(got / _sigma_with_prior(bare, precision[~free]) - 1).max()
    elsewhere = np.abs(got / _sigma_with_prior(bare, np.roll(precision, 6)[~free]) - 1).max()      # the prior on the wrist and 14 angles
    rescaled = np.abs(got / _sigma_with_prior(bare, 2 * precision[~free]) - 1).max()
    d = np.einsum("nii->ni", bare)
    share = (precision[~free] / d).max(1)
    lam = np.linalg.eigvalsh(bare / np.sqrt(d[:, :, None] * d[:, None, :]))[:, 0]
    ceiling = 1 - 1 / np.sqrt(1 + share / lam)
    print(f"sigma of the free angles vs angle_sigma {at_free:.1e} relative; the others move by {moved.max(1).min():.3f} .. {moved.max():.3f} "
          f"(largest share {share.max():.3f}; 1 - 1 / sqrt(1 + share / lambda_min) {ceiling.min():.3f} .. {ceiling.max():.3f}); against Woodbury "
          f"{exact:.1e}, with the prior on other columns {elsewhere:.1e}, at twice the precision {rescaled:.1e}")
    assert at_free <= 2.0 ** -21
    assert exact <= 1e-9 and elsewhere > 1e-3 and rescaled > 1e-3
    assert np.all(moved >= -1e-12) and np.all(moved.max(1) <= ceiling)
    assert np.abs(uc.information(c, drop=("prior",))["info"][:, 3] - uc.SINGULAR).max() == 0


# ----------------------------------------------------------------------------- calibration
MC_SIGMA_PX, MC_DRAWS, MC_BAND = 0.5, 1024, 5.0 * np.sqrt(2.0 / 1024)
MC_HANDS = (0, 9, 17, 28, 40, 63)


def _monte_carlo(name, hands, seed, sigma_px=MC_SIGMA_PX):
    """The float64 fit under the case's loss (max_iters 32, from the label pose) on MC_DRAWS noisy copies of each hand's windows,
    Gaussian noise of sigma_px, weights 1 / sigma^2: (the case of the hands, the landmark displacements [hands, draws, 21, 3] from
    the landmarks behind the exact windows)."""
    c = uc.subset(uc.case(name), hands)
    c["weights"] = (c["weights"] / sigma_px ** 2).astype(np.float32)
    k = len(hands)
    rep = np.repeat(np.arange(k), MC_DRAWS)
    big = uc.subset(c, rep)
    rng = np.random.default_rng(seed)
    big["window"] = big["window"] + rng.normal(0.0, sigma_px, big["window"].shape)
    ja, xf, info = rc.fit_views_robust(big["hm"], big["window"], big["cam_rows"], big["table"], big["weights"], (big["ja"], big["xf"]),
                                       big["mirror"], None, big["t_scale"], 32, c["loss"], c["loss_scale"])[:3]
    assert np.all(info[:, 3] == vc.CONVERGED), np.unique(info[:, 3], return_counts=True)
    moved = vc.landmarks(big, dict(ja=ja, xf=xf)) - big["truth"]
    return c, moved.reshape(k, MC_DRAWS, 21, 3)


def test_landmark_covariance_is_what_noisy_fits_scatter_by():
    """Six golden hands of two_views, 1024 draws each: for every landmark the empirical mean |dp|^2 over tr Sigma_l lies within
    1 +- 5 sqrt(2 / N) = 1 +- 0.221 - five standard errors of a sample variance, 126 comparisons.  A restatement that drops the
    pivot (H turns about the origin, G about the centroid) misses the band; one that drops psi misses it in
    test_under_geman_mcclure_the_covariance_carries_psi.  The fit has no prior, so no calibration run can see one: the prior is
    held to its exact perturbation in test_the_prior_is_the_whole_answer_where_nothing_is_observed."""
    c, moved = _monte_carlo("two_views", MC_HANDS, 3)
    want = uc.information(c)
    assert np.all(want["info"][:, 3] == uc.OK)
    ratio = (moved ** 2).sum(-1).mean(1) / np.einsum("nlaa->nl", want["landmark_cov"])
    sig = np.sqrt(np.einsum("nlaa->nl", want["landmark_cov"]))
    print(f"hands {MC_HANDS}, sigma {MC_SIGMA_PX} px, {MC_DRAWS} draws: empirical / predicted variance {ratio.min():.3f} .. {ratio.max():.3f} "
          f"(band 1 +- {MC_BAND:.3f}); predicted landmark sigma {sig.min():.2f} .. {sig.max():.2f} mm")
    assert np.all(np.abs(ratio - 1) <= MC_BAND)
    wrong = uc.information(c, drop=("pivot",))
    shifted = (moved ** 2).sum(-1).mean(1) / np.einsum("nlaa->nl", wrong["landmark_cov"])
    assert np.abs(shifted - 1).max() > MC_BAND


def test_depth_of_a_one_view_hand_is_what_noisy_fits_scatter_by():
    """One best_view hand: along the eye ray of its camera through the pivot, every landmark's empirical variance over
    ray^T Sigma_l ray lies in the same band; the depth sigma against the lateral one is printed."""
    c, moved = _monte_carlo("best_view", (17,), 5)
    want = uc.information(c)
    assert want["info"][0, 3] == uc.OK
    centre = tc._split(c["table"][c["cam_rows"][0, 0]], tc.FISHEYE62)[3]
    ray = want["pivot"][0] - centre
    ray /= np.linalg.norm(ray)
    along = np.einsum("a,lab,b->l", ray, want["landmark_cov"][0], ray)
    ratio = ((moved[0] @ ray) ** 2).mean(0) / along
    across = np.sqrt((np.einsum("laa->l", want["landmark_cov"][0]) - along) / 2)
    print(f"hand 17 in its best view: depth variance empirical / predicted {ratio.min():.3f} .. {ratio.max():.3f}; depth sigma "
          f"{np.sqrt(along).min():.2f} .. {np.sqrt(along).max():.2f} mm against lateral {across.min():.2f} .. {across.max():.2f} mm, "
          f"ratio median {np.median(np.sqrt(along) / across):.1f}")
    assert np.all(np.abs(ratio - 1) <= MC_BAND)


def test_under_geman_mcclure_the_covariance_carries_psi():
    """One golden hand of two_views with 2 detections of each view displaced by 40 px, fitted under Geman-McClure at 2 px on 1024
    noisy copies.  The noise is 0.25 px, not 0.5: the covariance is the reweighted problem's, without the loss's second-order term,
    which is right while the inliers' d^2 / c^2 stays small (here 2 sigma^2 / c^2 = 0.03).  Every landmark's empirical variance
    over tr Sigma_l lies in the band; for a restatement that drops psi - the displaced detections then count as information - it
    does not."""
    sigma_px = 0.25
    c, moved = _monte_carlo("outliers_geman_mcclure", (17,), 7, sigma_px)
    assert c["displaced"].sum() == 4
    want, wrong = uc.information(c), uc.information(c, drop=("psi",))
    assert want["info"][0, 3] == uc.OK
    empirical = (moved[0] ** 2).sum(-1).mean(0)
    ratio, without = empirical / np.einsum("laa->l", want["landmark_cov"][0]), empirical / np.einsum("laa->l", wrong["landmark_cov"][0])
    print(f"hand 17, Geman-McClure at {c['loss_scale']} px, sigma {sigma_px} px: empirical / predicted variance {ratio.min():.3f} .. {ratio.max():.3f}; "
          f"without psi {without.min():.3f} .. {without.max():.3f}")
    assert np.all(np.abs(ratio - 1) <= MC_BAND)
    assert np.abs(without - 1).max() > MC_BAND
