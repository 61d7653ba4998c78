"""CPU tests of the hand-scale fit (ut_fit_pose_scale / ut_pool_scale, csrc/fit_scale.hip): the numpy restatement of
tests/scale_cases.py that the GPU tests compare with - its 27-column Jacobian against finite differences, its recovery of
known scales, the calibration of its scale information, the user05 recordings with the generic model - and the C boundary."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import mesh_cases as mc
import scale_cases as sc
from absolutetrack_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec00():
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand = mc.label_poses(lab)
    every6 = np.concatenate([2 * np.arange(0, 369, 6), 2 * np.arange(0, 369, 6) + 1])       # every 6th frame, both hands
    return dict(hm=hm, ja=ja, xf=xf, hand=hand, every6=every6)


def _targets(r, sel, k):
    return sc.forward(r["hm"], np.full(len(sel), float(k)), r["ja"][sel, :20], fc.effective_wrist(r["xf"][sel], r["hand"][sel], 1.0, np.float64))


def test_jacobian_with_the_scale_column_matches_central_differences(rec00):
    """The 20 label poses of tests/test_fit_host.py's Jacobian test, both hands, model scales 0.9 and 1.2: all 27 columns
    against central differences (h = 1e-5) of the float64 forward function, to 1e-6 of a column's largest entry - the bound
    of the 26 columns there, for the reasons given there.  Measured: 1.0e-7 (the sigma column alone: 2.0e-8)."""
    sel = np.arange(0, 738, 37)[:20]
    assert set(rec00["hand"][sel]) == {0, 1}
    hm, ang = rec00["hm"], rec00["ja"][sel, :20].copy()
    m = fc.effective_wrist(rec00["xf"][sel], rec00["hand"][sel], 1.0, np.float64)
    s = np.where(np.arange(20) % 2 == 0, 0.9, 1.2)
    centroid = sc.forward(hm, s, ang, m).mean(1)
    jac = sc.jacobian(hm, s, ang, m, centroid)
    h, worst, worst_sigma = 1e-5, 0.0, 0.0
    for k in range(27):
        d = np.zeros((20, 27))
        d[:, k] = h
        pa, pm, ps = sc.apply_step(ang, m, s, centroid, d)
        na, nm, ns = sc.apply_step(ang, m, s, centroid, -d)
        fd = ((sc.forward(hm, ps, pa, pm) - sc.forward(hm, ns, na, nm)) / (2 * h)).reshape(20, 63)
        scale = np.abs(fd).max(1)
        assert np.all(scale > 0), k
        err = float((np.abs(jac[:, :, k] - fd).max(1) / scale).max())
        worst = max(worst, err)
        if k == 26:
            worst_sigma = err
    print(f"27-column Jacobian vs central differences: {worst:.3e} of a column's largest entry (sigma column {worst_sigma:.3e})")
    assert worst <= 1e-6


@pytest.mark.parametrize("k", [0.8, 1.0, 1.3])
def test_scale_recovery(rec00, k):
    """recording_00's model scaled by k, every 6th frame and both hands (124 poses), cold start with init_scale 1.
    float64: s to <= 1e-6, landmarks to <= 1e-5 mm, every pose converged.  float32: s to <= 4e-6 (1e-3 mm at a 250 mm hand).
    Measured: float64 |s - k| <= 3.4e-8, landmarks 3.6e-6 mm; float32 |s - k| <= 2.4e-7."""
    sel = rec00["every6"]
    tg = _targets(rec00, sel, k)
    ja, xf, s, info = sc.fit_scale(rec00["hm"], tg, mirror=rec00["hand"][sel])
    back = sc.forward(rec00["hm"], s, ja[:, :20], fc.effective_wrist(xf, rec00["hand"][sel], 1.0, np.float64))
    kp = np.linalg.norm(back - tg, axis=-1).max()
    print(f"k = {k}: float64 |s - k| {np.abs(s - k).max():.2e}, landmarks {kp:.2e} mm, iterations mean {info[:, 2].mean():.2f} max "
          f"{int(info[:, 2].max())}")
    assert np.all(info[:, 3] == sc.CONVERGED)
    assert np.abs(s - k).max() <= 1e-6 and kp <= 1e-5
    assert np.all(info[:, 4] > 0) and np.array_equal(info[:, 5], np.zeros(len(sel)))
    ja32, xf32, s32, info32 = sc.fit_scale(rec00["hm"], tg, mirror=rec00["hand"][sel], dtype=np.float32)
    print(f"k = {k}: float32 |s - k| {np.abs(s32.astype(np.float64) - k).max():.2e}, iterations max {int(info32[:, 2].max())}, information "
          f"float32 vs float64 {np.abs(info32[:, 4] / info[:, 4] - 1).max():.2e} relative")
    assert s32.dtype == np.float32 and np.all(info32[:, 3] == sc.CONVERGED)
    assert np.abs(s32.astype(np.float64) - k).max() <= 4e-6


def test_information_is_the_schur_complement_and_the_last_cholesky_pivot(rec00):
    """information() against the last pivot of a Cholesky factorisation of the same matrix (what the kernel computes), in
    float64 and with the factorisation in float32."""
    sel = rec00["every6"][::4]
    m = fc.effective_wrist(rec00["xf"][sel], rec00["hand"][sel], 1.0, np.float64)
    ang = rec00["ja"][sel, :20]
    tg = _targets(rec00, sel, 1.0)
    ones = np.ones((len(sel), 21))
    a_mat, _g = sc._normal(rec00["hm"], np.ones(len(sel)), ang, m, tg.mean(1), ones, ones > 0, tg, sc.FREE, np.float64)
    want = sc.information(a_mat)
    diag = np.einsum("bii->bi", a_mat)
    damped = a_mat + sc.SCALE_INFO_LAMBDA * np.einsum("bi,ij->bij", np.maximum(diag, fc.DIAG_FLOOR * diag.max(1, keepdims=True)), np.eye(27))
    piv64 = np.linalg.cholesky(damped)[:, 26, 26] ** 2
    piv32 = np.linalg.cholesky(damped.astype(np.float32))[:, 26, 26].astype(np.float64) ** 2
    print(f"last pivot^2 vs Schur complement: float64 {np.abs(piv64 / want - 1).max():.2e}, float32 factorisation "
          f"{np.abs(piv32 / want - 1).max():.2e} relative")
    assert np.abs(piv64 / want - 1).max() <= 1e-9 and np.abs(piv32 / want - 1).max() <= 1e-3
    singular = np.zeros((1, 27, 27))
    assert np.array_equal(sc.information(singular), [0.0])


@pytest.mark.parametrize("noise", [0.5, 2.0])
def test_information_is_calibrated(rec00, noise):
    """369 label poses (every frame, hands alternating), Gaussian noise of `noise` mm on every target coordinate, free fit
    started from the labels: (ln s - ln 1) sqrt(information) / noise has rms 1 when the information is the inverse
    variance it claims to be.  Asserted: rms in [0.9, 1.1].  Measured with this seed: 0.5 mm -> 1.008, 2 mm -> 1.030
    (the standard error of an rms over 369 samples is 0.037)."""
    sel = 2 * np.arange(369) + np.arange(369) % 2
    rng = np.random.default_rng(11)
    tg = _targets(rec00, sel, 1.0) + rng.normal(0, noise, (len(sel), 21, 3))
    ja, xf, s, info = sc.fit_scale(rec00["hm"], tg, init=(rec00["ja"][sel], rec00["xf"][sel]), mirror=rec00["hand"][sel])
    ok = sc.usable(s, info)
    z = np.log(s[ok]) * np.sqrt(info[ok, 4]) / noise
    rms = np.sqrt((z ** 2).mean())
    print(f"noise {noise} mm: {ok.sum()} of {len(sel)} usable, z rms {rms:.3f}, mean {z.mean():+.3f}; scale sd {np.log(s[ok]).std():.2e}")
    assert ok.sum() >= 0.98 * len(sel)
    assert 0.9 <= rms <= 1.1


@pytest.fixture(scope="module")
def user05(golden_dir):
    """The 305 valid hand-frames of the three user05 recordings, fitted with the GENERIC model in the float64 restatement:
    free pass, pool, fixed passes at 1, at the pooled scale and at the pooled scale x (1 -+ 0.0025)."""
    g = np.load(os.path.join(golden_dir, "fk_user05.npz"))
    generic = dict(np.load(pipeline._DATA.replace("recording_00_labels", "generic_hand_model")))
    kp, hand = [], []
    for rec in ("00", "02", "11"):
        valid = g[f"r{rec}.valid_tracking"]
        h, f = np.nonzero(valid)
        kp.append(g[f"r{rec}.gt_keypoints"][h, f])
        hand.append(h)
    kp, hand = np.concatenate(kp).astype(np.float64), np.concatenate(hand)
    free = sc.fit_scale(generic, kp, mirror=hand)
    pooled = sc.pool(free[2], free[3], len(kp))[0]
    fixed = {k: sc.fit_scale(generic, kp, init=(free[0], free[1]), init_scale=np.full(len(kp), k), mode=sc.FIXED, mirror=hand)
             for k in (1.0, pooled[0], pooled[0] * (1 - 0.0025), pooled[0] * (1 + 0.0025))}
    return dict(generic=generic, kp=kp, hand=hand, free=free, pooled=pooled, fixed=fixed)


def test_user05_generic_model_with_one_pooled_scale(user05):
    """The headline: the generic model times one pooled scale fits user05's stored keypoints better than the generic model as
    shipped, and the information-weighted pool of per-pose scales is the minimiser of the joint fixed-scale cost.
    Measured (float64): median rms residual 4.66 mm (max 5.19) as shipped -> 1.96 mm (max 2.96) at the pooled scale 1.0930;
    pooled scale vs the vertex of the parabola through the joint cost at 1.0930 x (1 - 0.0025, 1, 1 + 0.0025): 3.5e-6 (asserted:
    1e-4, 0.025 mm at a 250 mm hand); non-converged poses float64 0, float32 0 of 305 (asserted: at most 2 %)."""
    u = user05
    n = len(u["kp"])
    assert n == 305
    s, info = u["free"][2], u["free"][3]
    pooled = u["pooled"]
    used = sc.usable(s, info)
    not_converged = int(((info[:, 3].astype(int) & sc.CONVERGED) == 0).sum())
    assert pooled[3] == used.sum() and not_converged <= 0.02 * n and n - used.sum() <= 0.02 * n
    ks = sorted(u["fixed"])
    assert ks[0] == 1.0
    shipped, at_pooled = u["fixed"][1.0][3][:, 0], u["fixed"][pooled[0]][3][:, 0]
    cost = [float((21 * u["fixed"][k][3][used, 0] ** 2).sum()) for k in ks[1:]]
    x = np.log(np.array(ks[1:]))
    c2, c1, _c0 = np.polyfit(x - x[1], cost, 2)
    vertex = np.exp(x[1] - c1 / (2 * c2))
    print(f"user05, generic model: per-pose scales {s[used].min():.4f} .. {s[used].max():.4f}, pooled {pooled[0]:.5f} (sigma "
          f"{pooled[1]:.2e} per mm, scatter {pooled[2]:.3f} mm, {int(pooled[3])} poses, {not_converged} not converged); rms residual median "
          f"{np.median(shipped):.3f} (max {shipped.max():.3f}) mm as shipped -> {np.median(at_pooled):.3f} (max {at_pooled.max():.3f}) mm; "
          f"vertex of the joint cost {vertex:.6f}, pooled - vertex {pooled[0] - vertex:+.2e}")
    assert c2 > 0
    assert np.median(at_pooled) < np.median(shipped)
    assert abs(pooled[0] - vertex) <= 1e-4
    # the fixed passes kept their scale, bit for bit, and report no information
    for k in ks:
        assert np.array_equal(u["fixed"][k][2], np.full(n, k)) and np.array_equal(u["fixed"][k][3][:, 4], np.zeros(n))
    ja32, xf32, s32, info32 = sc.fit_scale(u["generic"], u["kp"], mirror=u["hand"], dtype=np.float32)
    nc32 = int(((info32[:, 3].astype(int) & sc.CONVERGED) == 0).sum())
    p32 = sc.pool(s32, info32, n)[0]
    print(f"float32 restatement: {nc32} not converged, pooled {p32[0]:.6f} ({p32[0] - pooled[0]:+.2e} from float64)")
    assert nc32 <= 0.02 * n


def test_observability(rec00):
    """A hand seen only at its wrist and fingertips says next to nothing about its scale - bent fingers explain a short hand:
    the information of such a pose is at most 1e-2 of the same pose with all landmarks (measured: 1.0e-4 at the most), and
    124 such poses added to a group of 124 full poses (1 mm noise on both) move the pooled scale by less than 1e-4
    (measured: 6e-9).  Three landmarks of one finger (5 wrist, 6, 7 thumb) are enough for the fit to converge."""
    sel = rec00["every6"]
    rng = np.random.default_rng(3)
    tg = _targets(rec00, sel, 1.0) + rng.normal(0, 1.0, (len(sel), 21, 3))
    init = (rec00["ja"][sel], rec00["xf"][sel])
    full = sc.fit_scale(rec00["hm"], tg, init=init, mirror=rec00["hand"][sel])
    w = np.zeros((len(sel), 21))
    w[:, :6] = 1                                       # landmarks 0..4 fingertips, 5 wrist
    tips = sc.fit_scale(rec00["hm"], tg, weights=w, init=init, mirror=rec00["hand"][sel])
    ratio = tips[3][:, 4] / full[3][:, 4]
    alone = sc.pool(full[2], full[3], len(sel))[0]
    both = sc.pool(np.concatenate([full[2], tips[2]]), np.concatenate([full[3], tips[3]]), 2 * len(sel))[0]
    print(f"wrist + fingertips only: information {ratio.max():.2e} of the full pose's at the most; status counts "
          f"{np.bincount(tips[3][:, 3].astype(int))}; pooled scale {alone[0]:.6f} -> {both[0]:.6f} with them ({both[0] - alone[0]:+.2e}), "
          f"poses used {int(alone[3])} -> {int(both[3])}")
    assert np.all(np.isfinite(tips[2])) and ratio.max() <= 1e-2
    assert abs(both[0] - alone[0]) < 1e-4
    w = np.zeros((len(sel), 21))
    w[:, 5:8] = 1
    three = sc.fit_scale(rec00["hm"], _targets(rec00, sel, 1.0), weights=w, init=init, mirror=rec00["hand"][sel])
    print(f"landmarks 5, 6, 7 only: status counts {np.bincount(three[3][:, 3].astype(int))}, iterations max {int(three[3][:, 2].max())}")
    assert np.all(three[3][:, 3].astype(int) & sc.CONVERGED) and np.isfinite(three[2]).all()


def test_pool_rules():
    """What a pool uses and what an empty group gives."""
    scale = np.array([1.1, 1.2, 0.9, 1.3, 1.0, 1.0])
    info = np.zeros((6, 6))
    info[:, 3] = [sc.CONVERGED, sc.AT_MAX_ITERS, sc.CONVERGED | sc.AT_BOUND, sc.CONVERGED, sc.REFUSED, sc.CONVERGED]
    info[:, 4] = [100, 100, 100, 300, 100, np.nan]
    out = sc.pool(scale, info, 3)
    assert np.array_equal(sc.usable(scale, info), [True, False, False, True, False, False])
    assert out[0, 3] == 1 and abs(out[0, 0] - 1.1) < 1e-15 and abs(out[0, 1] - 0.1) < 1e-15 and out[0, 2] < 1e-12
    assert out[1, 3] == 1 and abs(out[1, 0] - 1.3) < 1e-15
    assert np.array_equal(sc.pool(scale[:3], info[:3] * [1, 1, 1, 0, 1, 1], 3)[0], [1, np.inf, 0, 0])
    both = sc.pool(scale[[0, 3]], info[[0, 3]], 2)[0]
    mean = (100 * np.log(1.1) + 300 * np.log(1.3)) / 400
    want_scatter = np.sqrt(100 * (np.log(1.1) - mean) ** 2 + 300 * (np.log(1.3) - mean) ** 2)
    assert abs(both[0] - np.exp(mean)) < 1e-15 and abs(both[1] - 0.05) < 1e-15 and abs(both[2] - want_scatter) < 1e-15 and both[3] == 2


def test_restatement_refusals(rec00):
    """A bad init_scale refuses the pose like a bad weight does: scale 1, the rest pose, status REFUSED; the neighbours fit."""
    sel = rec00["every6"][:6]
    tg = _targets(rec00, sel, 1.0)
    init_scale = np.array([1.0, np.nan, 0.2, 4.5, np.inf, 1.0])
    ja, xf, s, info = sc.fit_scale(rec00["hm"], tg, init_scale=init_scale, mirror=rec00["hand"][sel])
    assert np.array_equal(info[:, 3], [sc.CONVERGED, sc.REFUSED, sc.REFUSED, sc.REFUSED, sc.REFUSED, sc.CONVERGED])
    assert np.array_equal(s[1:5], np.ones(4)) and np.array_equal(ja[1:5], np.zeros((4, 22))) and np.array_equal(info[1:5, 4], np.zeros(4))
    # targets of a model 8 times the size end at the upper bound and say so
    ja, xf, s, info = sc.fit_scale(rec00["hm"], _targets(rec00, sel[:2], 8.0), mirror=rec00["hand"][sel[:2]])
    assert np.array_equal(s, np.full(2, sc.SCALE_MAX)) and np.all(info[:, 3].astype(int) & sc.AT_BOUND) and np.isfinite(ja).all()


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_scale_entries_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "scale_c99.c"), "-o", str(tmp_path / "scale_c99.o")])


def test_scale_table_matches_the_scale_header():
    """What tests/test_fit_host.py checks for umetrack_hip_fit.h, for umetrack_hip_scale.h and the binding's scale table: every
    ut_* declaration of the header has one entry with as many argtypes as the C declaration has parameters, load_library()
    declares exactly those, no other header names them, and the constants of the binding, the restatement and the header
    agree."""
    from absolutetrack_amd import _native
    text = open(os.path.join(ROOT, "include", "umetrack_hip_scale.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_fit_pose_scale": 24, "ut_pool_scale": 8}
    assert set(declared) == set(_native.SCALE_EXPORTS)
    assert not set(declared) & (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS))
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._SCALE_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    for other in ("umetrack_hip.h", "umetrack_hip_fit.h", "umetrack_hip_triangulate.h"):
        assert not re.search(r"ut_fit_pose_scale|ut_pool_scale", open(os.path.join(ROOT, "include", other)).read()), other
    enums = dict(re.findall(r"\b(UT_(?:SCALE|FITS)_[A-Z_]+)\s*=\s*(\d+)", header))
    assert {k: int(v) for k, v in enums.items()} == dict(
        UT_SCALE_FREE=_native.UT_SCALE_FREE, UT_SCALE_FIXED=_native.UT_SCALE_FIXED, UT_FITS_CONVERGED=_native.UT_FITS_CONVERGED,
        UT_FITS_AT_MAX_ITERS=_native.UT_FITS_AT_MAX_ITERS, UT_FITS_REFUSED=_native.UT_FITS_REFUSED, UT_FITS_AT_BOUND=_native.UT_FITS_AT_BOUND)
    assert (sc.FREE, sc.FIXED, sc.CONVERGED, sc.AT_MAX_ITERS, sc.REFUSED, sc.AT_BOUND) == (0, 1, 1, 2, 4, 8)
    defines = {k: float(v) for k, v in re.findall(r"#define\s+(UT_SCALE_[A-Z_]+)\s+([0-9.e-]+)f", header)}
    assert defines == dict(UT_SCALE_MIN=sc.SCALE_MIN, UT_SCALE_MAX=sc.SCALE_MAX, UT_SCALE_INFO_LAMBDA=sc.SCALE_INFO_LAMBDA)
    assert (_native.UT_SCALE_MIN, _native.UT_SCALE_MAX) == (sc.SCALE_MIN, sc.SCALE_MAX)


def test_library_rejects_bad_scale_calls_on_the_host():
    """Argument validation happens before any device is touched: every UT_E_INVALID case of both entries, nothing launched,
    no pointer followed, nothing written."""
    from absolutetrack_amd import _native
    lib = _native.load_library()
    n = 4
    buf = {k: np.zeros(size, np.float32) for k, size in (("hm", 321), ("tg", n * 63), ("is", n), ("ia", n * 22), ("ix", n * 16), ("ja", n * 22),
                                                         ("xf", n * 16), ("s", n), ("info", n * 6), ("group", 8), ("ps", n))}
    p = {k: v.ctypes.data for k, v in buf.items()}
    good = dict(hm=p["hm"], n_models=1, tg=p["tg"], ts=63, w=None, lim=None, iscale=None, mode=0, ia=None, ias=22, ix=None, ixs=16,
                mirror=None, t_scale=1.0, iters=32, n=n, ja=p["ja"], jas=22, xf=p["xf"], xfs=16, s=p["s"], info=p["info"])

    def call(**change):
        a = dict(good, **change)
        rc = lib.ut_fit_pose_scale(None, a["hm"], a["n_models"], a["tg"], a["ts"], a["w"], a["lim"], a["iscale"], a["mode"], a["ia"],
                                   a["ias"], a["ix"], a["ixs"], a["mirror"], ctypes.c_float(a["t_scale"]), a["iters"], a["n"], a["ja"],
                                   a["jas"], a["xf"], a["xfs"], a["s"], a["info"], None)
        return rc, lib.ut_last_error(None).decode()

    for change in (dict(hm=None), dict(tg=None), dict(ja=None), dict(xf=None), dict(s=None),          # a null required pointer
                   dict(mode=2), dict(mode=-1),                                                         # an unknown scale_mode
                   dict(ia=p["ia"]), dict(ix=p["ix"]),                                                  # only one init pointer
                   dict(ts=62), dict(jas=21), dict(xfs=11),                                             # strides
                   dict(ia=p["ia"], ix=p["ix"], ias=21), dict(ia=p["ia"], ix=p["ix"], ixs=11),
                   dict(iters=0), dict(iters=257), dict(n_models=2), dict(n_models=0), dict(n=-1),
                   dict(t_scale=0.0), dict(t_scale=float("nan"))):
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("ut_fit_pose_scale: "), (change, rc, msg)
    assert call(n=0, hm=None, tg=None, ja=None, xf=None, s=None)[0] == 0        # nothing to do is not an error

    def pool(scale=p["s"], info=p["info"], n_groups=2, group_size=2, group=p["group"], pose_scale=p["ps"]):
        rc = lib.ut_pool_scale(None, scale, info, n_groups, group_size, group, pose_scale, None)
        return rc, lib.ut_last_error(None).decode()

    for change in (dict(scale=None), dict(info=None), dict(group=None), dict(n_groups=-1), dict(group_size=0), dict(group_size=-3)):
        rc, msg = pool(**change)
        assert rc == -1 and msg.startswith("ut_pool_scale: "), (change, rc, msg)
    assert pool(n_groups=0, scale=None, info=None, group=None)[0] == 0
    assert all(not b.any() for b in buf.values())                               # nothing was written
