"""CPU tests of the pose fit (ut_fit_pose, csrc/fit.hip): the float64 numpy solver of tests/fit_cases.py that the GPU tests
compare with - its Jacobian against finite differences, its recovery of the label poses - and the C boundary."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import mesh_cases as mc
from absolutetrack_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec00():
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand = mc.label_poses(lab)
    targets = fc.forward(hm, ja, fc.effective_wrist(xf, hand, 1.0, np.float64))
    return dict(hm=hm, ja=ja, xf=xf, hand=hand, targets=targets)


def test_jacobian_matches_central_differences(rec00):
    """20 label poses, both hands (right ones through the mirror, where the cross product changes sign).  Central
    differences on the float64 forward function with h = 1e-5: truncation ~ h^2 x the third derivative (1e-10 of a
    column), rounding ~ 1e-16 x 300 mm / h = 3e-9 mm per rad against columns of 10 .. 100 mm per rad.
    Measured: 1.0e-7 of the column's largest entry (worst over the 26 columns), the same for h = 1e-4 and 1e-6 - so it is
    not the differencing but the data: the labels' wrist rotations are orthogonal only as far as float32 stored them
    (|R^T R - I| = 6e-8, printed below), and the identity R (a x b) = det(R) (R a x R b) behind the world-space cross
    product holds for orthogonal R; the palm centre's float32 weights sum to 1 + 4e-8, which is the 1.5e-8 of the
    translation columns.  Asserted: 1e-6, ten times that, and what the label angles inside so3_exp_map's clamp
    (|angle| < 0.01 rad, where the analytic Jacobian deliberately differs) are kept out of: none of these poses has one."""
    sel = np.arange(0, 738, 37)[:20]
    assert len(sel) == 20 and set(rec00["hand"][sel]) == {0, 1}
    hm, ang = rec00["hm"], rec00["ja"][sel, :20].copy()
    m = fc.effective_wrist(rec00["xf"][sel], rec00["hand"][sel], 1.0, np.float64)
    centroid = rec00["targets"][sel].mean(1)
    jac = fc.jacobian(hm, ang, m, centroid)
    h = 1e-5
    worst = 0.0
    for k in range(26):
        d = np.zeros((len(sel), 26))
        d[:, k] = h
        plus = fc.forward(hm, *fc.apply_step(ang, m, centroid, d))
        minus = fc.forward(hm, *fc.apply_step(ang, m, centroid, -d))
        fd = ((plus - minus) / (2 * h)).reshape(len(sel), 63)
        scale = np.abs(fd).max(1)
        moving = scale > 0
        assert moving.any(), k
        worst = max(worst, float((np.abs(jac[:, :, k] - fd).max(1)[moving] / scale[moving]).max()))
        assert np.array_equal(jac[~moving, :, k], np.zeros_like(jac[~moving, :, k]))
    r = m[:, :3, :3]
    print(f"analytic Jacobian vs central differences: {worst:.3e} of a column's largest entry; |R^T R - I| of these wrists "
          f"{np.abs(r.transpose(0, 2, 1) @ r - np.eye(3)).max():.1e}, smallest |angle| {np.abs(ang).min():.4f} rad")
    assert np.abs(ang).min() > 0.01
    assert worst <= 1e-6


def test_float64_solver_recovers_the_label_poses(rec00):
    """All 738 label poses from the cold start, exact targets: <= 1e-5 mm on every landmark and <= 1e-6 rad on every angle
    (modulo 2 pi) within 16 iterations, every pose reporting convergence; the float32 yardstick beside it."""
    ja, xf, info = fc.fit(rec00["hm"], rec00["targets"], mirror=rec00["hand"], max_iters=16)
    back = fc.forward(rec00["hm"], ja, fc.effective_wrist(xf, rec00["hand"], 1.0, np.float64))
    kp = np.linalg.norm(back - rec00["targets"], axis=-1).max()
    ang = fc.angle_distance(ja[:, :20], rec00["ja"][:, :20]).max()
    print(f"float64 solver, 738 poses, cold start: {kp:.3e} mm, {ang:.3e} rad, at most {int(info[:, 2].max())} iterations")
    assert np.all(info[:, 3] == fc.CONVERGED) and info[:, 2].max() <= 16
    assert kp <= 1e-5 and ang <= 1e-6
    assert np.abs(ja[:, :20]).max() <= np.pi and np.array_equal(ja[:, 20:], np.zeros((738, 2)))
    # the wrist is the proper transform of the labels, for both hands
    assert np.abs(xf - rec00["xf"]).max() <= 1e-5 and np.all(np.linalg.det(xf[:, :3, :3]) > 0)
    assert info[:, 0].max() <= info[:, 1].max() <= 1e-5          # rms and worst residual as the solver saw them
    ja32, xf32, info32 = fc.fit(rec00["hm"], rec00["targets"], mirror=rec00["hand"], max_iters=16, dtype=np.float32)
    assert ja32.dtype == np.float32 and xf32.dtype == np.float32
    back = fc.forward(rec00["hm"], ja32.astype(np.float64), fc.effective_wrist(xf32, rec00["hand"], 1.0, np.float64))
    print(f"float32 yardstick: {np.linalg.norm(back - rec00['targets'], axis=-1).max():.3e} mm, "
          f"{fc.angle_distance(ja32[:, :20], rec00['ja'][:, :20]).max():.3e} rad, at most {int(info32[:, 2].max())} iterations")
    assert np.all(info32[:, 3] == fc.CONVERGED)


def test_solver_refuses_and_ignores_what_it_should(rec00):
    """Weight 0 hides a landmark completely (a NaN target there changes nothing, the fingertip's distal angle stays
    exactly 0 from a cold start); fewer than three weighted landmarks are refused with finite outputs."""
    sel = np.arange(0, 738, 74)
    tg = rec00["targets"][sel].copy()
    w = np.ones((len(sel), 21))
    tips = np.arange(len(sel)) % 5
    w[np.arange(len(sel)), tips] = 0
    tg[np.arange(len(sel)), tips] = np.nan
    ja, xf, info = fc.fit(rec00["hm"], tg, weights=w, mirror=rec00["hand"][sel], max_iters=24)
    assert np.all(info[:, 3] == fc.CONVERGED) and np.isfinite(ja).all() and np.isfinite(xf).all()
    assert np.array_equal(ja[np.arange(len(sel)), 4 * tips + 3], np.zeros(len(sel)))
    back = fc.forward(rec00["hm"], ja, fc.effective_wrist(xf, rec00["hand"][sel], 1.0, np.float64))
    assert np.linalg.norm(back - rec00["targets"][sel], axis=-1)[w > 0].max() <= 1e-5
    w[0] = 0
    w[0, :2] = 1
    ja, xf, info = fc.fit(rec00["hm"], tg, weights=w, mirror=rec00["hand"][sel], max_iters=24)
    assert info[0, 3] == fc.REFUSED and np.array_equal(ja[0], np.zeros(22)) and np.array_equal(xf[0], np.eye(4))
    assert np.all(info[1:, 3] == fc.CONVERGED)


def test_header_declares_the_fit_entry_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "fit_c99.c"), "-o", str(tmp_path / "fit_c99.o")])


def test_extension_table_matches_the_extension_header():
    """What tests/test_host_logic.py checks for umetrack_hip.h and the core table, for umetrack_hip_fit.h and the binding's
    extension table: every ut_* declaration of the header has one entry with as many argtypes as the C declaration has
    parameters, load_library() declares exactly those, and the core header does not name the entry."""
    import re
    from absolutetrack_amd import _native
    header = open(os.path.join(ROOT, "include", "umetrack_hip_fit.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_fit_pose": 21}
    assert set(declared) == set(_native.EXTENSION_EXPORTS) and not set(declared) & set(_native.EXPORTS)
    lib = _native.load_library()
    for name, (restype, argtypes) in _native._EXTENSION_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert "ut_fit_pose" not in open(os.path.join(ROOT, "include", "umetrack_hip.h")).read()


def test_library_exports_the_fit_entry_and_rejects_on_the_host():
    """Argument validation happens before any device is touched, so the refusals can be checked here: nothing is launched
    and no pointer is followed."""
    from absolutetrack_amd import _native
    lib = _native.load_library()
    assert "ut_fit_pose" in _native.EXTENSION_EXPORTS and "ut_fit_pose" not in _native.EXPORTS and hasattr(lib, "ut_fit_pose")
    n = 4
    buf = {k: np.zeros(size, np.float32) for k, size in (("hm", 321), ("tg", n * 63), ("ia", n * 22), ("ix", n * 16),
                                                         ("ja", n * 22), ("xf", n * 16), ("info", n * 4))}
    good = dict(hm=buf["hm"].ctypes.data, n_models=1, tg=buf["tg"].ctypes.data, ts=63, w=None, lim=None, ia=None, ias=22, ix=None,
                ixs=16, mirror=None, t_scale=1.0, iters=32, n=n, ja=buf["ja"].ctypes.data, jas=22, xf=buf["xf"].ctypes.data, xfs=16,
                info=buf["info"].ctypes.data)

    def call(**change):
        a = dict(good, **change)
        rc = lib.ut_fit_pose(None, a["hm"], a["n_models"], a["tg"], a["ts"], a["w"], a["lim"], a["ia"], a["ias"], a["ix"], a["ixs"],
                             a["mirror"], ctypes.c_float(a["t_scale"]), a["iters"], a["n"], a["ja"], a["jas"], a["xf"], a["xfs"],
                             a["info"], None)
        return rc, lib.ut_last_error(None).decode()

    for change in (dict(hm=None), dict(tg=None), dict(ja=None), dict(xf=None),                       # a null required pointer
                   dict(ia=buf["ia"].ctypes.data), dict(ix=buf["ix"].ctypes.data),                    # only one init pointer
                   dict(ts=62), dict(jas=21), dict(xfs=11),                                           # strides
                   dict(ia=buf["ia"].ctypes.data, ix=buf["ix"].ctypes.data, ias=21),
                   dict(ia=buf["ia"].ctypes.data, ix=buf["ix"].ctypes.data, ixs=11),
                   dict(iters=0), dict(iters=257), dict(n_models=2), dict(n_models=0), dict(n=-1),
                   dict(t_scale=0.0), dict(t_scale=float("nan"))):
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("ut_fit_pose: "), (change, rc, msg)
    assert call(n=0, hm=None, tg=None, ja=None, xf=None)[0] == 0            # nothing to do is not an error
    assert all(not b.any() for b in buf.values())                           # nothing was written
