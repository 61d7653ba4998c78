"""CPU tests of the start of a pose fit in the views (ut_start_pose_views, ut_select_pose, include/umetrack_hip_start.h): the C
boundary, the bank and the seeds, and the numpy restatement of tests/start_cases.py that the GPU tests compare with - its
translation is the dense least-squares solution, its refusals are the header's, and on the 74 golden hands the chain start -> fit
-> selection finds the hand from the detections alone.  DESIGN.md, "Start of a pose fit in the views"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import start_cases as sc
import step_cases as st
import views_cases as vc
from absolutetrack_amd import _native, hand, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the C boundary
def test_header_declares_the_entries_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "start_c99.c"), "-o", str(tmp_path / "start_c99.o")])


def test_prototype_table_matches_the_header():
    """Each ut_* declaration of umetrack_hip_start.h has one entry in the binding's table of its own with as many argtypes as the C
    declaration has parameters, load_library() declares it, and no older table names it."""
    text = open(os.path.join(ROOT, "include", "umetrack_hip_start.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = {}
    for name, params in re.findall(r"\b(ut_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in declared, name
        declared[name] = params.count(",") + 1
    assert declared == {"ut_start_pose_views": 25, "ut_select_pose": 14}
    assert set(declared) == set(_native.START_EXPORTS)
    older = (set(_native.EXPORTS) | set(_native.EXTENSION_EXPORTS) | set(_native.TRIANGULATE_EXPORTS) | set(_native.SCALE_EXPORTS)
             | set(_native.INFO_EXPORTS) | set(_native.VIEWS_EXPORTS) | set(_native.ROBUST_EXPORTS) | set(_native.VIEWS_SCALE_EXPORTS)
             | set(_native.UNCERTAINTY_EXPORTS) | set(_native.SMOOTH_EXPORTS))
    assert not set(declared) & older
    lib = _native.load_library()
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    for name, (restype, argtypes) in _native._START_PROTOTYPES.items():
        assert declared[name] == len(argtypes), (name, declared[name], len(argtypes))
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # handle | model | window weights cam_rows max_views table n_rows kind | limits | bank | seeds | mirror t_scale iters n | pose out | info | stream
    assert list(_native._START_PROTOTYPES["ut_start_pose_views"][1]) == \
        [vp, vp, i32] + [vp, vp, vp, i32, vp, i32, i32] + [vp] + [vp, i32] + [vp, i32] + [vp, f32, i32, i32] + [vp, i32, vp, i32] + [vp] + [vp]
    assert list(_native._START_PROTOTYPES["ut_select_pose"][1]) == [vp, i32, vp, i32, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp]
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(UT_START_[A-Z_]+)\s+(\d+)\s", header)}
    assert codes == dict(UT_START_MAX_SEEDS=64) and _native.UT_START_MAX_SEEDS == 64
    assert '#include "umetrack_hip_views.h"' in text


def test_library_rejects_on_the_host():
    """Argument validation happens before any device is touched: nothing is launched and no pointer is followed."""
    lib = _native.load_library()
    bufs = dict(hm=np.ones(321, np.float32), win=np.ones(2 * 2 * 42), rows=np.zeros(4, np.int32), tab=np.ones(32), bank=np.zeros(40, np.float32),
                seeds=np.tile(np.eye(3).reshape(9), 3), ja=np.zeros(4 * 22, np.float32), xf=np.zeros(4 * 16, np.float32))
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, n_models=1, max_views=2, n_rows=1, kind=0, n_bank=2, n_seeds=3, t_scale=1.0, iters=30,
                n=2, ja_stride=22, xf_stride=16)

    def call(**change):
        a = dict(good, **change)
        rc = lib.ut_start_pose_views(None, a["hm"], a["n_models"], a["win"], None, a["rows"], a["max_views"], a["tab"], a["n_rows"], a["kind"], None,
                                     a["bank"], a["n_bank"], a["seeds"], a["n_seeds"], None, ctypes.c_float(a["t_scale"]), a["iters"], a["n"],
                                     a["ja"], a["ja_stride"], a["xf"], a["xf_stride"], None, None)
        return rc, lib.ut_last_error(None).decode()

    for change, word in ((dict(hm=None), "null"), (dict(win=None), "null"), (dict(rows=None), "null"), (dict(tab=None), "null"), (dict(bank=None), "null"),
                         (dict(seeds=None), "null"), (dict(ja=None), "null"), (dict(xf=None), "null"), (dict(kind=2), "table_kind"),
                         (dict(max_views=0), "max_views"), (dict(max_views=9), "max_views"), (dict(n_rows=0), "bad argument"), (dict(n=-1), "bad argument"),
                         (dict(n_models=3), "bad argument"), (dict(n_bank=0), "n_bank"), (dict(n_seeds=0), "n_seeds"), (dict(n_seeds=65), "n_seeds"),
                         (dict(iters=0), "iters"), (dict(iters=257), "iters"), (dict(ja_stride=21), "stride"), (dict(xf_stride=11), "stride"),
                         (dict(t_scale=0.0), "t_scale"), (dict(t_scale=float("nan")), "t_scale"), (dict(n=0, n_seeds=0), "n_seeds")):
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("ut_start_pose_views: ") and word in msg, (change, rc, msg)
    assert call(n=0, n_models=1)[0] == 0                                               # nothing to do is not an error
    assert not bufs["ja"].any() and not bufs["xf"].any()

    info = np.zeros(8, np.float32)
    for args, word in (((None, 22, bufs["xf"].ctypes.data, 16, info.ctypes.data, 1, 2, bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16), "null"),
                       ((bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16, None, 1, 2, bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16), "null"),
                       ((bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16, info.ctypes.data, 1, 0, bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16), "bad"),
                       ((bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16, info.ctypes.data, -1, 2, bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16), "bad"),
                       ((bufs["ja"].ctypes.data, 21, bufs["xf"].ctypes.data, 16, info.ctypes.data, 1, 2, bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16), "stride"),
                       ((bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16, info.ctypes.data, 1, 2, bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 11), "stride")):
        rc = lib.ut_select_pose(*args, None, None, None)
        msg = lib.ut_last_error(None).decode()
        assert rc == -1 and msg.startswith("ut_select_pose: ") and word in msg, (args, rc, msg)
    assert lib.ut_select_pose(bufs["ja"].ctypes.data, 22, bufs["xf"].ctypes.data, 16, info.ctypes.data, 0, 2, bufs["ja"].ctypes.data, 22,
                              bufs["xf"].ctypes.data, 16, None, None, None) == 0


# ----------------------------------------------------------------------------- the bank and the seeds
def test_bank_and_seeds():
    """The bank is the zero pose plus the fractions of the limits, inside the box; the seeds are 24 distinct proper signed
    permutations with the identity first; the package's and the restatement's agree."""
    lim = st.joint_limits()
    b = sc.bank()
    assert b.shape == (4, 20) and b.dtype == np.float32 and not b[0].any()
    assert np.all(b[1:] >= lim[:, 0]) and np.all(b[1:] <= lim[:, 1])
    assert np.allclose(b[2], 0.5 * (lim[:, 0] + lim[:, 1]), atol=1e-6)
    q = sc.seeds()
    assert q.shape == (24, 3, 3) and np.array_equal(q[0], np.eye(3))
    assert np.allclose(np.linalg.det(q), 1.0) and np.array_equal(q @ q.transpose(0, 2, 1), np.tile(np.eye(3), (24, 1, 1)))
    assert set(np.unique(q)) == {-1.0, 0.0, 1.0} and len({m.tobytes() for m in q}) == 24
    assert np.array_equal(hand.start_rotation_seeds().numpy(), q)
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    assert np.array_equal(hand.start_pose_bank(model).numpy(), b)
    assert np.array_equal(hand.start_pose_bank(model, (0.5,)).numpy(), b[[0, 2]])
    assert hand.start_pose_bank(model._replace(joint_limits=None)).shape == (1, 20)


# ----------------------------------------------------------------------------- one step, the refusals
def test_translation_is_the_dense_least_squares_solution():
    """Given R, the closed translation is the minimiser of sum w |A (R p + t - o)|^2: numpy's lstsq on the stacked 3 O x 3 system."""
    c = sc.golden_case("two", 0)
    rays = sc.Rays(c["window"], c["cam_rows"], c["table"], c["weights"])
    p = sc.rigid_shape(c["hm"], np.zeros((74, 20), np.float32), c["mirror"])
    rot = np.einsum("bij,sjk->bsik", rays.rot, sc.seeds()[:3])
    po = p[:, rays.lm]
    rp = np.einsum("bsij,boj->bsoi", rot, po)
    t = rays.translation(rp, ~rays.refused)
    worst = 0.0
    for b in range(0, 74, 9):
        a = np.eye(3) - rays.d[b, :, :, None] * rays.d[b, :, None, :]
        sw = np.sqrt(rays.w[b])[:, None, None]
        for s in range(3):
            rhs = -(sw * a @ (rp[b, s] - rays.o[b])[..., None]).reshape(-1)
            dense = np.linalg.lstsq((sw * a).reshape(-1, 3), rhs, rcond=None)[0]
            worst = max(worst, np.abs(dense - t[b, s]).max() / max(1.0, np.abs(dense).max()))
    print(f"translation against lstsq: {worst:.2e} relative")
    assert worst <= 1e-9
    # a round does not raise the ray cost (orthogonal iteration descends)
    def ray_cost(r, tt):
        z = np.einsum("bsij,boj->bsoi", r, po) + tt[:, :, None] - rays.o[:, None]
        az = z - rays.d[:, None] * (rays.d[:, None] * z).sum(-1, keepdims=True)
        return (rays.w[:, None] * (az * az).sum(-1)).sum(-1)
    r1, t1 = sc.iterate(rays, p, rot, 1)
    r2, t2 = sc.iterate(rays, p, rot, 2)
    assert np.all(ray_cost(r2, t2) <= ray_cost(r1, t1) * (1 + 1e-12)) and np.all(ray_cost(r1, t1) <= ray_cost(rot, t) * (1 + 1e-12))


def test_refusals_of_the_restatement():
    """A negative weight, a NaN window at a positive weight, two used landmarks, and three landmarks on one ray (sum w A singular) are
    refused: the bank pose at the identity wrist, info (0, 0, -1, REFUSED); a NaN window at weight 0 changes nothing; a bad
    cam_rows entry raises."""
    c = vc.subset(dict(sc.golden_case("two", 0), init=(np.zeros((74, 22), np.float32), np.zeros((74, 4, 4), np.float32))), np.arange(6))
    win, w = c["window"].copy(), c["weights"].copy()
    seen = np.argwhere(w[0, 0] > 0)[:, 0]
    w[1, 0, seen[0]] = -1.0
    win[2, 0, seen[0], 1] = np.nan
    w[3] = 0
    w[3, 0, seen[:2]] = 1
    w[4] = 0
    w[4, 0, seen[:3]] = 1
    win[4, 0, seen[:3]] = win[4, 0, seen[0]]
    w[5, 1, 4] = 0
    win[5, 1, 4] = np.nan
    args = (c["hm"], win, c["cam_rows"], c["table"], sc.bank()[:2], sc.seeds()[:4], w, c["mirror"])
    r = sc.start_pose_views(*args, iters=5)
    info = r["info"].reshape(6, 2, 4)
    assert np.array_equal(info[1:5], np.tile(np.float32([0, 0, -1, sc.REFUSED]), (4, 2, 1)))
    assert np.all(info[[0, 5], :, 3] == 0) and np.all(info[[0, 5], :, 2] >= 0)
    assert np.array_equal(r["xf"].reshape(6, 2, 4, 4)[1:5], np.tile(np.eye(4, dtype=np.float32), (4, 2, 1, 1)))
    assert np.array_equal(r["ja"].reshape(6, 2, 22)[:, :, :20], np.tile(sc.bank()[:2], (6, 1, 1)))
    clean = win.copy()
    clean[5, 1, 4] = 0.0
    again = sc.start_pose_views(c["hm"], clean, *args[2:], iters=5)
    assert all(np.array_equal(r[k], again[k]) for k in ("ja", "xf", "info"))
    rows = c["cam_rows"].copy()
    rows[0, 1] = len(c["table"])
    with pytest.raises(IndexError):
        sc.start_pose_views(c["hm"], win, rows, *args[3:])


def test_select_pose_restatement():
    info = np.float32([[3, 0, 1, 1], [2, 0, 1, 4], [2.5, 0, 1, 2], [2.5, 0, 1, 1],      # the refused 2 px loses; the first 2.5 wins the tie
                       [0, 0, 0, 4], [0, 0, 0, 4], [0, 0, 0, 4], [0, 0, 0, 4],          # all refused
                       [np.nan, 0, 1, 1], [1, 0, 1, 1], [np.inf, 0, 1, 1], [1, 0, 1, 1]])
    ja = np.arange(12 * 22, dtype=np.float32).reshape(12, 22)
    xf = np.arange(12 * 16, dtype=np.float32).reshape(12, 4, 4)
    a, x, i, index = sc.select_pose(ja, xf, info, 4)
    assert index.tolist() == [2, -1, 1] and index.dtype == np.int32
    assert np.array_equal(a, ja[[2, 4, 9]]) and np.array_equal(x, xf[[2, 4, 9]]) and np.array_equal(i[:2], info[[2, 4]])


# ----------------------------------------------------------------------------- the yardstick on the 74 golden hands
@pytest.mark.parametrize("views", ["two", "one"])
def test_cold_chain_finds_the_golden_hands(views):
    """Bank of 4, 24 seeds, 30 rounds, float64 fits of 64 iterations from every start, selection - nothing but the detections.
    Exact golden windows: the selected pose's worst landmark within BASIN_MM = 5 mm of the golden landmarks on all 74 hands in two
    views, on at least 72 with the best view alone (73 measured: the missing hand sits in a mirror pose of the kind
    views_cases.full_case describes).  With 1 px noise (default_rng(0)) the criterion is the cost's: the selected rms <= 1.05 x the
    rms of the fit started at the label + 0.01 px, on at least 72 hands (measured 74 in two views, 73 in one)."""
    c = sc.golden_case(views, 0)
    r = sc.cold_fit(c)
    found = int((sc.landmark_error(c, r) <= sc.BASIN_MM).sum())
    print(f"{views} views, exact windows: {found} / 74 selected poses within {sc.BASIN_MM} mm; candidates chosen {np.bincount(r['index'], minlength=4)}")
    assert found == 74 if views == "two" else found >= 72
    cn = sc.golden_case(views, 1.0)
    rn = sc.cold_fit(cn)
    good = int(sc.rms_criterion(cn, rn).sum())
    print(f"{views} views, 1 px noise: {good} / 74 selected rms within 1.05 x the label-started fit's + 0.01 px")
    assert good >= 72


# ----------------------------------------------------------------------------- the documented loss
def test_recovery_rule_on_the_documented_loss():
    """DESIGN.md "Poses smoothed over a sequence": hand 1 of frames 200..263, two views, 0.5 px (seed 5 + hand), warm-started from the
    previous fit, loses the hand (11.9 mm rms against the labels; 1.556 mm when every frame starts at its label).  With
    tracker.track_hand_poses_in_views' rule at its default ratio - measured, float64: frames 23, 28 and 31 take the cold result and the
    sequence's rms falls to 4.68 mm.  Frame 23 comes back to the hand; at frames 28 and 31 the cold chain itself ends 95 mm off at
    1.57 px rms, where the label-started fit has 0.55 px and the warm fit 4.3 px: better than the warm fit by the cost, not the hand.
    Warm rms / cold rms is 1.000 on every frame where the warm fit sits on the hand and 8.06, 2.75 and 2.74 at the three lost frames.
    Asserted is what that supports: the rule's sequence is not worse than warm-only, and every frame's chosen rms <= its warm rms."""
    import fit_cases as fc
    import smooth_cases as sm
    seq = sm.recording(200, 263, 1, 2, 0.5)
    c = dict(seq["views_case"], limits=None)
    truth = fc.forward(c["hm"], seq["truth_ja"].astype(np.float64)[:, :20], fc.effective_wrist(seq["truth_xf"].astype(np.float64), c["mirror"], 1.0, np.float64))

    def rms_mm(res):
        return float(np.sqrt((np.linalg.norm(vc.landmarks(c, res) - truth, axis=-1) ** 2).mean()))

    cold = sc.cold_fit(c, max_iters=32)
    init = (seq["truth_ja"][:1], seq["truth_xf"][:1])
    warm_only, ruled = sc.track(c, cold, init, None), sc.track(c, cold, init)
    ratio = ruled["warm_rms"] / cold["info"][:, 0]
    print(f"warm-only {rms_mm(warm_only):.3f} mm, with the rule {rms_mm(ruled):.3f} mm, cold alone {rms_mm(cold):.3f} mm; recovered frames "
          f"{np.flatnonzero(ruled['recovered']).tolist()}; warm / cold rms there {ratio[ruled['recovered']].round(2).tolist()}, elsewhere at most "
          f"{ratio[~ruled['recovered']].max():.4f}")
    assert not warm_only["recovered"].any() and ruled["recovered"].any()
    assert rms_mm(ruled) <= rms_mm(warm_only)
    assert np.all(ruled["info"][:, 0] <= ruled["warm_rms"].astype(np.float32) + 1e-6)
