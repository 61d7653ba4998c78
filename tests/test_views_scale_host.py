"""CPU tests of the pose fit in the views with the hand's scale as a parameter (ut_fit_pose_views_scale,
include/umetrack_hip_views_scale.h): the C boundary, and the numpy restatement of tests/views_scale_cases.py that the GPU tests
compare with - its 63 reduced rows with 27 columns give the stacked normal equations, with the scale fixed it is
views_cases.fit_views on the scaled model, free it recovers the scale of exact two-view windows, one view carries no scale
information, and on noisy detections it beats the 3-D chain it starts from.

Measured, float64, the 74 golden hands (python -m pytest tests/test_views_scale_host.py -s prints the figures): DESIGN.md, "Hand
scale from keypoints in the views"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import scale_cases as sc
import views_cases as vc
import views_scale_cases as vs
from absolutetrack_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "umetrack_hip_views_scale.h"


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "views_scale_c99.c"), "-o", str(tmp_path / "views_scale_c99.o")])


def test_prototype_table_matches_the_header():
    """The ut_* declaration of umetrack_hip_views_scale.h has one entry in the binding's table of its own with as many argtypes
    as the C declaration has parameters, load_library() declares it, no other header or table names it, and its argument list is
    ut_fit_pose_views_robust's with (init_scale, scale_mode) behind limits and scale in front of info."""
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_fit_pose_views_scale": 32}
    assert set(declared) == set(_native.VIEWS_SCALE_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS) | set(_native.VIEWS_EXPORTS) | set(_native.ROBUST_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._VIEWS_SCALE_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    robust = list(_native._ROBUST_PROTOTYPES["ut_fit_pose_views_robust"][1])
    assert list(_native._VIEWS_SCALE_PROTOTYPES["ut_fit_pose_views_scale"][1]) == \
        robust[:11] + [ctypes.c_void_p, ctypes.c_int32] + robust[11:25] + [ctypes.c_void_p] + robust[25:]
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER:
            assert "ut_fit_pose_views_scale" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert '#include "umetrack_hip_robust.h"' in text and '#include "umetrack_hip_scale.h"' in text
    assert "one camera cannot see the hand's size" in text.lower()


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed.  What
    ut_fit_pose_views_robust refuses under the entry's own name, an unknown scale_mode and a null scale."""
    lib = _native.load_library()
    n, v = 3, 2
    hm, win, w = np.zeros(321, np.float32), np.zeros(n * v * 42), np.zeros(n * v * 21, np.float32)
    rows, table = np.zeros(n * v, np.int32), np.zeros(4 * 32)
    ja, xf, info, s = np.zeros(n * 22, np.float32), np.zeros(n * 16, np.float32), np.zeros(n * 6, np.float32), np.zeros(n, np.float32)
    res, inl = np.zeros(n * v * 21, np.float32), np.zeros(n * v * 21, np.float32)
    ija, ixf, isc = np.ones(n * 22, np.float32), np.ones(n * 16, np.float32), np.ones(n, np.float32)
    good = dict(hm=hm.ctypes.data, n_models=1, win=win.ctypes.data, w=w.ctypes.data, rows=rows.ctypes.data, v=v, table=table.ctypes.data,
                n_rows=4, kind=0, isc=isc.ctypes.data, mode=0, ija=ija.ctypes.data, ija_stride=22, ixf=ixf.ctypes.data, ixf_stride=16,
                t_scale=1.0, iters=32, loss=0, scale=3.0, n=n, ja=ja.ctypes.data, ja_stride=22, xf=xf.ctypes.data, xf_stride=16,
                s=s.ctypes.data, info=info.ctypes.data, res=res.ctypes.data, inl=inl.ctypes.data)

    def fit(**change):
        a = dict(good, **change)
        rc_ = lib.ut_fit_pose_views_scale(None, a["hm"], a["n_models"], a["win"], a["w"], a["rows"], a["v"], a["table"], a["n_rows"],
                                          a["kind"], None, a["isc"], a["mode"], a["ija"], a["ija_stride"], a["ixf"], a["ixf_stride"], None,
                                          ctypes.c_float(a["t_scale"]), a["iters"], a["loss"], ctypes.c_float(a["scale"]), a["n"], a["ja"],
                                          a["ja_stride"], a["xf"], a["xf_stride"], a["s"], a["info"], a["res"], a["inl"], None)
        return rc_, lib.ut_last_error(None).decode()

    for change in (dict(mode=2), dict(mode=-1), dict(s=None), dict(n=0, s=None), dict(n=0, mode=2), dict(loss=3), dict(loss=-1),
                   dict(loss=1, scale=0.0), dict(loss=2, scale=float("nan")), dict(ija=None), dict(ixf=None), dict(hm=None),
                   dict(win=None), dict(rows=None), dict(table=None), dict(ja=None), dict(xf=None), dict(n=-1), dict(n_models=2),
                   dict(v=0), dict(v=9), dict(kind=2), dict(n_rows=0), dict(ja_stride=21), dict(xf_stride=11), dict(iters=0),
                   dict(iters=257), dict(t_scale=0.0)):
        code, msg = fit(**change)
        assert code == -1 and msg.startswith("ut_fit_pose_views_scale: "), (change, code, msg)
    assert "scale_mode must be" in fit(mode=7)[1] and "loss must be" in fit(loss=7)[1] and "no cold start" in fit(ija=None, ixf=None)[1]
    assert fit(n=0)[0] == 0 and fit(n=0, mode=1, loss=1)[0] == 0           # nothing to do is not an error
    assert fit(n=0, isc=None, inl=None, res=None, info=None)[0] == 0       # init_scale and three outputs are optional
    assert not any(b.any() for b in (ja, xf, info, s, res, inl))           # nothing was written
    with pytest.raises(ValueError):
        _native.fit_pose_views_scale(None, None, None, None, None, None, scale_mode=2)


# ----------------------------------------------------------------------------- the restatement
def _state(c, s):
    vw = vs.rc.views_of(c)
    ang = c["init"][0].astype(np.float64)[:, :20]
    m = fc.effective_wrist(c["init"][1], c["mirror"], c["t_scale"], np.float64)
    centroid = vc.pivot(vw, fc.forward(sc.scaled_model(c["hm"], s), ang, m, np.float64), np.float64)[0]
    return vw, ang, m, centroid


@pytest.mark.parametrize("name", vs.STEP_CASES)
def test_reduced_rows_give_the_stacked_normal_equations(name):
    """J^T J and J^T r of the 63 reduced rows with 27 columns are those of the stacked 2 V 21 reprojection rows whose sigma column
    is J_v (p - t) per view: float64, at the cases' starts and start scale, 1e-9 of the largest entry."""
    worst = 0.0
    for k in vs.SCALES:
        c = vs.case(name, k)
        s = np.asarray(c["init_scale"], np.float64)
        vw, ang, m, centroid = _state(c, s)
        idx = np.arange(len(s))
        jr, rr = vs.reduced_system(vw, c["hm"], s, ang, m, centroid, idx, vs.FREE, np.float64)
        js, rs = vs.stacked_system(vw, c["hm"], s, ang, m, centroid, idx)
        for got, want in ((jr.transpose(0, 2, 1) @ jr, js.transpose(0, 2, 1) @ js),
                          ((jr.transpose(0, 2, 1) @ rr[..., None])[..., 0], (js.transpose(0, 2, 1) @ rs[..., None])[..., 0])):
            rel = np.abs(got - want).reshape(len(s), -1).max(1) / np.abs(want).reshape(len(s), -1).max(1)
            worst = max(worst, float(rel.max()))
        fixed = vs.reduced_system(vw, c["hm"], s, ang, m, centroid, idx, vs.FIXED, np.float64)[0]
        assert not fixed[:, :, 26].any() and np.array_equal(fixed[:, :, :26], jr[:, :, :26])
    print(f"\n{name}: reduced against stacked normal equations, 27 columns: {worst:.1e} relative")
    assert worst <= 1e-9


def test_fixed_mode_is_fit_views_on_the_scaled_model():
    """With the scale fixed at 1.1 the restatement is views_cases.fit_views on scaled_model(hm, 1.1): float64, equal iteration
    counts, poses to 1e-10, information 0 and the scale returned as given."""
    c = vs.case("two_views", 1.25)
    s = np.full(len(c["mirror"]), np.float32(1.1))
    got = vs.restate(dict(c, mode=vs.FIXED, init_scale=s), np.float64, 32)
    want = vc.restate(dict(c, hm=sc.scaled_model(c["hm"], s.astype(np.float64))), np.float64, 32)
    d_ja, d_xf = np.abs(got["ja"] - want["ja"]).max(), np.abs(got["xf"] - want["xf"]).max()
    print(f"\nfixed at 1.1 against fit_views on the scaled model: {d_ja:.1e} rad, {d_xf:.1e} mm, "
          f"iterations {got['info'][:, 2].max():.0f} / {want['info'][:, 2].max():.0f}")
    assert np.array_equal(got["info"][:, 2:4], want["info"][:, 2:4])
    assert d_ja <= 1e-10 and d_xf <= 1e-10 and np.abs(got["residual"] - want["residual"]).max() <= 1e-6
    assert np.array_equal(got["scale"], s.astype(np.float64)) and not got["info"][:, 4:].any()


@pytest.mark.parametrize("name", vs.STEP_CASES)
def test_free_mode_recovers_the_scale(name):
    """Exact windows of the model scaled by k, starts +-0.2 rad / +-15 mm at scale 1, float64: every hand converges, none at a
    bound, the scale within SCALE_TOL of k."""
    for k in vs.SCALES:
        c = vs.case(name, k)
        r = vs.restate(c, np.float64, 32)
        status = r["info"][:, 3].astype(np.int64)
        err = np.abs(r["scale"] - k).max()
        print(f"\n{name} x {k}: scale within {err:.1e}, at most {r['info'][:, 2].max():.0f} iterations, information "
              f"{r['info'][:, 4].min():.3g} .. {r['info'][:, 4].max():.3g}")
        assert np.all(status == vs.CONVERGED) and err <= vs.SCALE_TOL and np.all(r["info"][:, 4] > 0)


def test_decisions_of_the_restatement():
    """A start scale that is not finite or outside the bounds refuses the pose: scale 1, the start comes back, information 0."""
    c = vs.subset(vs.case("two_views", 0.8), np.arange(5))
    c["init_scale"] = np.array([np.nan, 0.1, 5.0, 1.0, np.inf], np.float32)
    r = vs.restate(c, np.float64, 8)
    refused = np.array([True, True, True, False, True])
    assert np.array_equal((r["info"][:, 3].astype(np.int64) & vs.REFUSED) != 0, refused)
    assert np.all(r["scale"][refused] == 1) and not r["info"][refused][:, [0, 1, 2, 4, 5]].any()
    assert np.array_equal(r["ja"][refused], c["init"][0][refused].astype(np.float64)) and not r["residual"][refused].any()


def test_one_camera_cannot_see_the_scale():
    """The best view alone, free, float64: every hand converges to a scale that means nothing with an information below 1e-3 of
    the same hand's two-view information, and pooling the 74 one-view fits with the 74 two-view fits as one group moves
    ln(pooled scale) by less than 1e-4."""
    for k in vs.SCALES:
        two, one = vs.restate(vs.case("two_views", k), np.float64, 32), vs.restate(vs.case("best_view", k), np.float64, 32)
        ratio = one["info"][:, 4] / two["info"][:, 4]
        alone = sc.pool(two["scale"], two["info"], 74)[0]
        both = sc.pool(np.concatenate([two["scale"], one["scale"]]), np.concatenate([two["info"], one["info"]]), 148)[0]
        moved = abs(np.log(both[0]) - np.log(alone[0]))
        print(f"\nx {k}: one view rms {one['info'][:, 0].max():.1e} px, scale off by up to {np.abs(one['scale'] - k).max():.3f}, information "
              f"{one['info'][:, 4].min():.3g} .. {one['info'][:, 4].max():.3g} against {two['info'][:, 4].min():.3g} .. "
              f"{two['info'][:, 4].max():.3g} in two views (ratio at most {ratio.max():.1e}); pooled with them ln s moves {moved:.1e} "
              f"({both[3]:.0f} poses used)")
        assert np.all(ratio < 1e-3) and moved < 1e-4


def test_views_fit_beats_the_chain_on_noisy_windows():
    """1 px noise on the two seeing views, the model at 1.1, seeds 0 - 2, starts from the float64 3-D chain (triangulation ->
    free scale fit): the views fit's per-pose rms of ln(s / 1.1) is below the chain's and its pool uses at least as many
    poses."""
    for seed in range(3):
        c = vs.noisy_case(1.0, seed)
        ch = c["chain"]
        r = vs.restate(c, np.float64, 32)
        use_c, use_v = sc.usable(ch["scale"], ch["info"]), sc.usable(r["scale"], r["info"])
        rms_c = np.sqrt((np.log(ch["scale"][use_c] / vs.NOISY_SCALE) ** 2).mean())
        rms_v = np.sqrt((np.log(r["scale"][use_v] / vs.NOISY_SCALE) ** 2).mean())
        pool_c, pool_v = sc.pool(ch["scale"], ch["info"], 74)[0], sc.pool(r["scale"], r["info"], 74)[0]
        print(f"\nseed {seed}: per-pose rms ln(s / 1.1) chain {rms_c:.4f} ({use_c.sum()} poses usable), views {rms_v:.4f} "
              f"({use_v.sum()} usable); pooled scale error chain {abs(pool_c[0] - vs.NOISY_SCALE):.4f}, views "
              f"{abs(pool_v[0] - vs.NOISY_SCALE):.4f}")
        assert rms_v < rms_c and use_v.sum() >= use_c.sum()
