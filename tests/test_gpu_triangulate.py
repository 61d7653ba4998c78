"""GPU tests of the triangulation (csrc/triangulate.hip through ut_triangulate_points and the Python layers above it) against
the reference's own numbers and the float64 numpy restatement of tests/triangulate_cases.py, which
tests/test_triangulate_host.py checks.

Bounds against the restatement: points 1e-9 mm, sigma 1e-6 relative, rms and per-view residuals 1e-6 px, status bits and view
counts equal.  Kernel and restatement evaluate the same expressions in the same order without contraction; what differs is the
last bit of atan2 / sin / cos / pow, i.e. ~1e-13 px in a window and ~1e-12 mm in a point."""
import numpy as np
import pytest
import torch

import fit_cases as fc
import mesh_cases as mc
import triangulate_cases as tc
from absolutetrack_amd import _native, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINT_TOL_MM, SIGMA_RTOL, PX_TOL = 1e-9, 1e-6, 1e-6
KP_TOL_MM, ANGLE_TOL_RAD = 1e-3, 1e-4


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _run(case, **kw):
    """ut_triangulate_points on a case of numpy arrays -> device tensors (points, info, residual)."""
    out = _native.triangulate_points(_t(case["window"]), _t(case["cam_rows"], torch.int32), _t(case["table"]),
                                     weights=None if case.get("weights") is None else _t(case["weights"], torch.float32), **kw)
    torch.cuda.synchronize()
    return out


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _compare(got, want, what, noisy=None):
    """The bounds of the module docstring; prints what it measured.  noisy: a mask [n,P] of points whose windows are not exact.
    Their minimum has a residual, and a trial is accepted only when the cost goes down: a step whose decrease the cost cannot
    resolve is rejected on one side and taken on the other, whichever way the last bits fall.  The stop rule of the header
    (UT_TRI_FLAT_TOL_PX) bounds what is left: a change of eps px in an rms residual of rho px is a step of
    sigma sqrt(2 eps rho), so such points are held to that instead of 1e-9 mm - the other bounds stay."""
    pts, info, res = got
    w_pts, w_info, w_res = want[:3]
    dist = np.linalg.norm(pts - w_pts, axis=-1)
    if noisy is not None:
        slack = w_info[..., 1].astype(np.float64) * np.sqrt(2 * tc.FLAT_TOL_PX * w_info[..., 0].astype(np.float64))
        print(f"{what}: {int(noisy.sum())} noisy point(s): {float(dist[noisy].max()):.3e} mm against {float(slack[noisy].min()):.3e} mm")
        assert np.all(dist[noisy] <= slack[noisy])
        dist = np.where(noisy, 0.0, dist)
    d_pts = float(dist.max())
    fin = np.isfinite(w_info[..., 1])
    d_sigma = float((np.abs(info[..., 1][fin].astype(np.float64) - w_info[..., 1][fin]) / w_info[..., 1][fin]).max()) if fin.any() else 0.0
    d_rms = float(np.abs(info[..., 0].astype(np.float64) - w_info[..., 0]).max())
    d_res = float(np.abs(res.astype(np.float64) - w_res).max())
    print(f"{what}: points {d_pts:.3e} mm, sigma {d_sigma:.3e} relative, rms {d_rms:.3e} px, residual {d_res:.3e} px; "
          f"status counts {np.bincount(info[..., 3].astype(int).ravel())}")
    assert np.isfinite(pts).all() and np.isfinite(res).all() and not np.isnan(info).any()
    assert np.array_equal(info[..., 3], w_info[..., 3]) and np.array_equal(info[..., 2], w_info[..., 2])
    assert np.array_equal(np.isposinf(info[..., 1]), np.isposinf(w_info[..., 1]))
    assert d_pts <= POINT_TOL_MM and d_sigma <= SIGMA_RTOL and d_rms <= PX_TOL and d_res <= PX_TOL


@pytest.fixture(scope="module")
def golden():
    g = tc.golden_case()
    g["want"] = tc.triangulate(g["window"], g["cam_rows"], g["table"], g["weights"])
    return g


@pytest.fixture(scope="module")
def rec00():
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand_idx = mc.label_poses(lab)
    blob = _t(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"], hm["landmark_rest_positions"],
                                      hm["landmark_rest_bone_weights"], hm["landmark_rest_bone_indices"]), torch.float32).reshape(-1, 321)
    return dict(lab=lab, hm=hm, ja=ja, xf=xf, hand=hand_idx, blob=blob, frame=np.arange(738) // 2)


# ----------------------------------------------------------------------------- 1. against the reference
def test_golden_points_match_the_reference_and_the_restatement(golden):
    """74 x 21 points in one launch, table = the 37 x 4 camera rows: the reference's landmarks from the reference's windows."""
    assert golden["table"].shape == (148, 32) and golden["window"].shape == (74, 4, 21, 2)
    got = _np(_run(golden))
    err = float(np.linalg.norm(got[0] - golden["landmarks"], axis=-1).max())
    print(f"ut_triangulate_points vs the reference's landmarks, 74 x 21 points: {err:.3e} mm")
    assert err <= POINT_TOL_MM
    assert np.all(got[1][..., 3] == _native.TRI_CONVERGED) and np.all(got[1][..., 2] == 2)
    _compare(got, golden["want"], "golden case vs the restatement")


# ----------------------------------------------------------------------------- 2. round trip on the device
def test_round_trip_fk_project_triangulate(rec00):
    """40 label poses of both hands: ut_fk -> ut_project_points -> weights from flags == 3 -> ut_triangulate_points comes back
    to the fk landmarks (fp32; everything in between is fp64) within 1e-3 mm; points_f32 written into [n,123] records."""
    r = rec00
    sel = np.arange(0, 738, 17)[:40]
    assert len(sel) == 40 and set(r["hand"][sel]) == {0, 1}
    lm = _native.fk_stateless(r["blob"], _t(r["ja"][sel], torch.float32), _t(r["xf"][sel], torch.float32), mirror=_t(r["hand"][sel], torch.int64))
    c = pipeline.label_candidates(r["lab"], r["frame"][sel])
    table = _t(c["cam_params"])
    rows = torch.arange(40 * 4, dtype=torch.int32, device=DEV).reshape(40, 4)
    win, _, flags = pipeline.project_keypoints(lm, table, rows, c["src_wh"])
    weights = (flags == 3).float()
    assert torch.equal(weights.sum(1), torch.full((40, 21), 2.0, device=DEV))          # every landmark in exactly two cameras
    rec = torch.full((40, 123), -7.0, device=DEV)
    pts, info, res = pipeline.triangulate_keypoints(win, table, rows, weights=weights, out_f32=rec[:, 60:], point_stride=123)
    torch.cuda.synchronize()
    err = float((pts - lm.double()).norm(dim=-1).max())
    print(f"fk -> project -> triangulate, 40 poses: {err:.3e} mm; sigma {float(info[..., 1].min()):.2f} .. {float(info[..., 1].max()):.2f} mm / px")
    assert err <= KP_TOL_MM
    assert bool((info[..., 3] == _native.TRI_CONVERGED).all()) and bool((info[..., 2] == 2).all())
    assert torch.equal(rec[:, 60:].reshape(40, 21, 3), pts.float()) and bool((rec[:, :60] == -7).all())
    assert bool((res[weights == 0] == 0).all())
    # the f32 output alone
    only = torch.zeros(40, 63, device=DEV)
    p2, _, _ = _native.triangulate_points(win, rows, table, weights=weights, out_f32=only, point_stride=63)
    assert torch.equal(only.reshape(40, 21, 3), pts.float()) and torch.equal(p2, pts)


# ----------------------------------------------------------------------------- 3. smallest shapes, ragged geometry
@pytest.mark.parametrize("n,n_pts,n_views,kind", [(1, 1, 2, tc.FISHEYE62), (3, 21, 2, tc.FISHEYE62), (13, 5, 4, tc.FISHEYE62),
                                                  (1, 21, 8, tc.FISHEYE62), (3, 21, 2, tc.PINHOLE), (13, 5, 4, tc.PINHOLE)])
def test_small_and_ragged_shapes(n, n_pts, n_views, kind):
    """Synthetic ring cameras with recording_00's intrinsics (and the same poses as pinhole crop cameras): 2, 3, 4 and 8 used
    views, -1 holes in the middle of cam_rows rows, zero weights with NaN windows in the first view."""
    case = tc.ragged_case(n, n_pts, n_views, kind, seed=n + n_views)
    want = tc.triangulate(case["window"], case["cam_rows"], case["table"], case["weights"])
    assert np.all(want[1][..., 3] == tc.CONVERGED) and np.linalg.norm(want[0] - case["points"], axis=-1).max() <= POINT_TOL_MM
    used = set(np.unique(want[1][..., 2]).astype(int))
    assert used == {(1, 2): {2}, (3, 2): {2}, (13, 4): {2, 3, 4}, (1, 8): {8}}[(n, n_views)]
    got = _np(_run(case))
    _compare(got, want, f"n {n}, points {n_pts}, views {n_views}, kind {kind}")
    assert np.linalg.norm(got[0] - case["points"], axis=-1).max() <= POINT_TOL_MM
    unused = (case["cam_rows"] < 0)[:, :, None] | (case["weights"] == 0)
    assert np.all(got[2][unused] == 0)


# ----------------------------------------------------------------------------- 4. batch independence
def test_batch_independence_and_determinism():
    case = tc.ragged_case(26, 21, 4, seed=5)
    rng = np.random.default_rng(5)
    case["window"] = case["window"] + 0.3 * rng.standard_normal(case["window"].shape)       # noisy: residuals and rejections
    whole = _run(case)
    again = _run(case)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    assert bool((whole[1][..., 3] == _native.TRI_CONVERGED).all())

    def part(sl):
        rows = case["cam_rows"][sl]
        return _run(dict(window=case["window"][sl], cam_rows=rows, table=case["table"], weights=case["weights"][sl]))
    for a, b in ((slice(0, 13), slice(13, 26)),):
        for sl in (a, b):
            assert all(torch.equal(x, y[sl]) for x, y in zip(part(sl), whole))
    for i in range(26):
        assert all(torch.equal(x, y[i:i + 1]) for x, y in zip(part(slice(i, i + 1)), whole)), i


# ----------------------------------------------------------------------------- 5. decisions
def test_decisions_on_the_device():
    cases = tc.decision_cases()
    got = {}
    for name, c in cases.items():
        want = tc.triangulate(c["window"], c["cam_rows"], c["table"], c["weights"])
        got[name] = _np(_run(c))
        pts, info, res = got[name]
        assert np.array_equal(info[..., 3], want[1][..., 3]) and np.array_equal(info[..., 2], want[1][..., 2]), name
        assert np.isfinite(pts).all() and np.isfinite(res).all() and not np.isnan(info).any(), name
        dead = (info[..., 3].astype(int) & (tc.REFUSED | tc.DEGENERATE)) != 0
        assert np.all(pts[dead] == 0) and np.all(np.isposinf(info[..., 1][dead])) and np.all(info[..., 0][dead] == 0), name
        assert np.all(res.transpose(0, 2, 1)[dead] == 0) and np.isfinite(info[..., 1][~dead]).all(), name
        noisy = None
        if name == "outlier":
            noisy = np.zeros((1, 21), bool)
            noisy[0, 7] = True
        _compare(got[name], want, name, noisy)
    assert np.all(got["one_view"][1][..., 3] == tc.REFUSED) and np.all(got["same_camera_twice"][1][..., 3] == tc.DEGENERATE)
    assert got["negative_weight"][1][0, 3, 3] == tc.REFUSED and got["nan_at_weight_1"][1][0, 5, 3] == tc.REFUSED
    assert all(np.array_equal(a, b) for a, b in zip(got["nan_at_weight_0"], got["garbage_at_weight_0"]))
    assert np.array_equal(got["nan_at_weight_0"][0], got["clean"][0])
    r = got["outlier"][2]
    assert np.unravel_index(np.argmax(r), r.shape) == (0, 2, 7)
    assert np.linalg.norm(got["outlier_zeroed"][0][0] - cases["clean"]["landmarks"], axis=-1).max() <= POINT_TOL_MM


# ----------------------------------------------------------------------------- 6. index check
def test_index_check():
    case = tc.ragged_case(4, 5, 3, seed=9)
    clean = _run(case)
    bad = dict(case, cam_rows=case["cam_rows"].copy())
    bad["cam_rows"][2, 1] = case["table"].shape[0]
    out = (torch.full((4, 5, 3), -7.0, dtype=torch.float64, device=DEV), torch.full((4, 5, 4), -7.0, device=DEV),
           torch.full((4, 3, 5), -7.0, device=DEV))
    with pytest.raises(IndexError, match="ut_triangulate_points"):
        _run(bad, out=out)
    torch.cuda.synchronize()
    keep = [0, 1, 3]
    assert all(bool((o[2] == -7).all()) for o in out)                       # the pose with the bad row wrote nothing
    assert all(torch.equal(o[keep], c[keep]) for o, c in zip(out, clean))   # the others are the clean run's
    bad["cam_rows"][2, 1] = -2
    with pytest.raises(IndexError, match="ut_triangulate_points"):
        _run(bad)
    assert all(torch.equal(a, b) for a, b in zip(_run(case), clean))        # and the device stays usable
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            for o in out:
                o.fill_(-7.0)
            _run(bad, out=out, engine=eng)                                  # returns: nothing synchronises in deferred mode
            assert all(bool((o[2] == -7).all()) for o in out) and all(torch.equal(o[keep], c[keep]) for o, c in zip(out, clean))
            with pytest.raises(IndexError, match="index check"):
                eng.poll_status()
            _run(case, out=out, engine=eng)
            eng.poll_status()
            assert all(torch.equal(o, c) for o, c in zip(out, clean))
    finally:
        eng.close()


# ----------------------------------------------------------------------------- 7. the chain into the pose fit
def test_hand_pose_from_window_keypoints(rec00):
    """20 label poses of both hands: the float64 FK landmarks projected on the host (float64) into the frame's four cameras,
    weights from visibility -> triangulation -> pose fit.  The bounds tests/test_gpu_fit.py asserts for exact targets."""
    r = rec00
    sel = np.arange(0, 738, 37)[:20]
    assert len(sel) == 20 and set(r["hand"][sel]) == {0, 1}
    hand_model = pipeline.hand_model_from_labels(r["lab"])
    targets = fc.forward(r["hm"], r["ja"][sel], fc.effective_wrist(r["xf"][sel], r["hand"][sel], 1.0, np.float64))
    worst_kp = worst_ang = worst_tri = 0.0
    for k, pose in enumerate(sel):
        cams = pipeline.cameras_for_frame(r["lab"], int(r["frame"][pose]))
        table = np.stack([tracker.geometry.pack_camera_model(c) for c in cams])
        win, ez = tc.project(table[:, None], targets[k][None], tc.FISHEYE62)
        weights = ((ez > 0) & (win >= 0).all(-1) & (win[..., 0] < cams[0].width) & (win[..., 1] < cams[0].height)).astype(np.float32)
        assert np.all(weights.sum(0) == 2)
        got, info = tracker.hand_pose_from_window_keypoints(hand_model, cams, win, int(r["hand"][pose]), weights=weights)
        assert got.hand_confidence == 1.0 and info.shape == (21, 4) and np.all(info[:, 3] == _native.TRI_CONVERGED)
        pts, _ = tracker.triangulate_landmarks(cams, win, weights)
        worst_tri = max(worst_tri, float(np.linalg.norm(pts - targets[k], axis=-1).max()))
        back = _native.fk_stateless(r["blob"], _t(got.joint_angles[None], torch.float32), _t(got.wrist_xform[None], torch.float32),
                                    mirror=_t(r["hand"][pose:pose + 1], torch.int64)).cpu().numpy()[0]
        worst_kp = max(worst_kp, float(np.linalg.norm(back.astype(np.float64) - targets[k], axis=-1).max()))
        worst_ang = max(worst_ang, float(fc.angle_distance(got.joint_angles[None, :20], r["ja"][pose:pose + 1, :20]).max()))
    print(f"window keypoints -> pose, 20 poses: triangulation {worst_tri:.3e} mm, ut_fk of the pose {worst_kp:.3e} mm, angles {worst_ang:.3e} rad")
    assert worst_tri <= POINT_TOL_MM and worst_kp <= KP_TOL_MM and worst_ang <= ANGLE_TOL_RAD
