"""GPU tests of the pose fit on 2-D keypoints in camera views (csrc/fit_views.hip through ut_fit_pose_views,
hand.fit_landmarks_views, tracker.refine_hand_pose_in_views and hand_pose_from_window_keypoints(refine_in_views=True)) against the
float64 / float32 numpy restatement of tests/views_cases.py, which tests/test_views_host.py checks.  The shapes are the 74 golden
hands and slices of 1 and 5.

Bounds (views_cases.bounds_from, DESIGN.md "One step against float64"): the project's 1e-4 rad and 1e-3 mm where the float32
restatement stays within a quarter of them, else 4 x the distance between the float32 and the float64 restatement on that
case - the worse of the two float32 solvers of step_cases.SOLVERS, computed here from the restatements, never from the
kernel's output, and printed.  rms and worst of info, in px, have no project bound: 4 x the float32 restatement's distance.
Measured distances: DESIGN.md, "Pose from keypoints in the views"."""
import numpy as np
import pytest
import torch

import step_cases as st
import triangulate_cases as tc
import views_cases as vc
from absolutetrack_amd import _native, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(*(hm[k] for k in st.FIELDS))).reshape(-1, 321)


def _gpu(c, max_iters, xf_stride=16, pad_views=0):
    """The case on the GPU -> numpy dict(ja [n,22], xf [n,4,4], info [n,4], residual [n,V,21]).  xf_stride = 12: the wrist is
    written as 12 floats per pose into a buffer with a guard row behind it, which must stay as it was.  pad_views: that many
    unused view slots (-1, NaN windows, NaN weights) behind the case's."""
    n, v = c["cam_rows"].shape
    win, rows, w = c["window"], c["cam_rows"], c["weights"]
    if pad_views:
        win = np.concatenate([win, np.full((n, pad_views, 21, 2), np.nan)], 1)
        rows = np.concatenate([rows, np.full((n, pad_views), -1, np.int32)], 1)
        w = np.concatenate([w, np.full((n, pad_views, 21), np.nan, np.float32)], 1)
    kw = dict(t_scale=c["t_scale"], max_iters=max_iters, residual=True)
    guard = None
    if xf_stride != 16:
        guard = torch.full((n + 1, xf_stride), 7.0, device=DEV)
        kw.update(n=n, out=(torch.empty(n, 22, device=DEV), guard), xf_stride=xf_stride)
    ja, xf, info, res = _native.fit_pose_views(_blob(c["hm"]), _t(win, torch.float64), _t(rows, torch.int32), _t(c["table"], torch.float64),
                                               _t(c["init"][0]), _t(c["init"][1]), None if w is None else _t(w),
                                               None if c["limits"] is None else _t(c["limits"]), _t(c["mirror"], torch.int64), **kw)
    torch.cuda.synchronize()
    xf = xf.cpu().numpy()
    if guard is not None:
        assert np.array_equal(xf[n], np.full(xf_stride, 7.0, np.float32))
        xf = np.concatenate([xf[:n, :12].reshape(n, 3, 4), np.tile(np.float32([[[0, 0, 0, 1]]]), (n, 1, 1))], 1)
    res = res.cpu().numpy()
    if pad_views:
        assert not res[:, v:].any()
        res = res[:, :v]
    return dict(ja=ja.cpu().numpy(), xf=xf.reshape(n, 4, 4), info=info.cpu().numpy(), residual=res)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("ja", "xf", "info", "residual"))


def _show(what, d, tol):
    print(f"{what}: angles {d['ang']:.2e} (bound {tol['ang']:.2e}) rad, landmarks {d['kp']:.2e} ({tol['kp']:.2e}) mm, rms / worst "
          f"{d['px']:.2e} ({tol['px']:.2e}) px")


# ----------------------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("name", vc.STEP_CASES)
def test_one_step(name):
    """max_iters = 1 from the +-0.2 rad / +-15 mm starts of the 74 golden hands, left and right: the 20 angles, the wrist, rms
    and worst against the float64 restatement's one step, landmarks through the float64 forward function of both; one iteration,
    the restatement's status; angles 20 and 21 copied through; the residuals of the returned pose."""
    c = vc.case(name)
    n = len(c["mirror"])
    assert set(c["mirror"]) == {0, 1}
    trace = []
    want = vc.restate(c, np.float64, 1, trace=trace)
    got = _gpu(c, 1, xf_stride=12 if name == "metres" else 16)
    d, tol = vc.distance(c, got, want), vc.bounds_from(vc.float32_distance(c, want))
    _show(f"one step, {name}", d, tol)
    assert trace[0]["accept"].all()
    assert np.array_equal(got["info"][:, 2], np.ones(n, np.float32))
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32))
    assert np.array_equal(_bits(got["ja"][:, 20:]), _bits(c["init"][0][:, 20:]))
    assert np.array_equal(got["xf"][:, 3], np.tile(np.float32([0, 0, 0, 1]), (n, 1)))
    assert vc.within(d, tol), (d, tol)
    used = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64).used
    assert not got["residual"][~used].any()
    assert np.abs(got["residual"] - want["residual"]).max() <= tol["px"] + tol["kp"] * _px_per_mm(c)


def _px_per_mm(c):
    """The largest norm of d window / d landmark over the case's used observations at its truth: px per mm."""
    vw = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64)
    jacs = vw.blocks(c["truth"], np.arange(len(c["truth"])))[6]
    return float(max(np.linalg.norm(j, axis=(-2, -1)).max() for j in jacs))


# ----------------------------------------------------------------------------- 2. full fits
@pytest.mark.parametrize("views", ["two", "one"])
def test_full_fits_on_exact_windows(views):
    """Full fits (max_iters = 32) on the reference's own windows from +-0.4 rad / +-30 mm, two views and the best view alone:
    every hand converges; landmarks against the golden landmarks by the bound rule (the float32 distance is the float32
    restatements' own from those landmarks); per pose at most the float32 restatements' iterations plus the margin - the largest
    distance of a float32 count from the float64 one, at least 2.
    Measured, MI355X: two views 8.5e-5 mm (float32 restatements 1.3e-4, float64 8.9e-5), iterations mean 6.1 max 9; one view
    3.9e-4 mm (3.1e-4, 1.8e-4), mean 6.5 max 11; margin 3 on both, largest GPU - float32 count 3 on both: at the rule's edge.  On
    exact windows the cost ends at the resolution of the fp32 landmarks, where rounding accepts or rejects a trial and every
    accepted one keeps the fit going, so the count's tail is geometric; a kernel variant with the projection out of line was one
    iteration over on 2 of the 148 poses ("Pose from keypoints in the views")."""
    c = vc.full_case(views)
    it32, it64, margin, runs = vc.full_yardstick(views)
    got = _gpu(c, 32)
    err = lambda r: float(np.linalg.norm(vc.landmarks(c, r) - c["truth"], axis=-1).max())
    d32 = max(err(runs[0]), err(runs[1]))
    bound = st.KP_TOL_MM if d32 <= st.KP_TOL_MM / 4 else st.FLOAT32_FACTOR * d32
    its = got["info"][:, 2].astype(np.int64)
    print(f"{views} view(s): GPU worst landmark {err(got):.2e} mm (bound {bound:.2e}; float32 restatements {d32:.2e}, float64 {err(runs[2]):.2e}), "
          f"rms up to {got['info'][:, 0].max():.1e} px; iterations GPU mean {its.mean():.1f} max {its.max()}, float32 max {it32.max()}, float64 "
          f"max {it64.max()}, margin {margin}, largest GPU - float32 {int((its - it32).max())}")
    assert np.array_equal(got["info"][:, 3], np.full(74, _native.UT_FIT_CONVERGED, np.float32))
    assert err(got) <= bound
    assert np.all(its <= it32 + margin)


# ----------------------------------------------------------------------------- 3. decisions
def _decision_case():
    c = vc.subset(vc.case("two_views"), np.arange(8))
    win, w, rows = c["window"].copy(), c["weights"].copy(), c["cam_rows"].copy()
    w[0, 1, 4] = 0
    win[0, 1, 4] = np.nan                         # a NaN window at weight 0
    w[1, 0, 3] = -1.0                             # a negative weight
    w[2, 1, 7] = np.nan                           # a NaN weight
    win[3, 0, 5, 1] = np.inf                      # a non-finite window at a positive weight
    w[4] = 0
    w[4, 0, [2, 9]] = 1                           # two landmarks with a used observation
    rows[5, 1] = -1
    w[5, 1] = np.nan                              # the weights of an unused view are not read
    return dict(c, window=win, weights=w, cam_rows=rows)


def test_refusals_keep_the_start_and_nan_at_weight_0_is_garbage_at_weight_0():
    c = _decision_case()
    got, want = _gpu(c, 32), vc.restate(c, np.float64, 32)
    assert np.array_equal(got["info"][:, 3].astype(int), [1, 4, 4, 4, 4, 1, 1, 1])
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32))
    for k in ("ja", "xf", "info", "residual"):
        assert np.isfinite(got[k]).all(), k
    assert np.array_equal(_bits(got["ja"][1:5]), _bits(c["init"][0][1:5])) and np.array_equal(_bits(got["xf"][1:5]), _bits(c["init"][1][1:5]))
    assert not got["info"][1:5, :3].any() and not got["residual"][1:5].any() and not got["residual"][5, 1].any()
    err = np.linalg.norm(vc.landmarks(c, got) - c["truth"], axis=-1).max(1)
    assert err[[0, 5, 6, 7]].max() <= st.KP_TOL_MM
    garbage = c["window"].copy()
    garbage[0, 1, 4] = 123.5
    assert _same_bits(got, _gpu(dict(c, window=garbage), 32))


def test_padding_and_batches_leave_the_bits():
    """max_views 4 with two unused slots gives the bits of max_views 2 (3 -> 5 on the ragged case, whose hole lies in the
    middle); a pose alone, in a batch of 5 and in the batch of 74 - across the workgroups of 4 poses - gives the same bits."""
    for name in ("two_views", "ragged"):
        c = vc.case(name)
        whole = _gpu(c, 32)
        assert _same_bits(whole, _gpu(c, 32, pad_views=2)), name
        for sel in (np.array([41]), np.arange(6, 11)):
            assert _same_bits(_gpu(vc.subset(c, sel), 32), {k: v[sel] for k, v in whole.items()}), (name, sel)


def _behind(c, i):
    """The case with pose i's start mirrored through the image plane of its first pinhole view: behind the camera."""
    cam = c["table"][c["cam_rows"][i, 0]]
    axis = cam[4:13].reshape(3, 3)[:, 2]
    xf = c["init"][1].copy()
    xf[i, :3, 3] -= (2 * (axis @ (c["truth"][i].mean(0) - cam[13:16])) * axis).astype(np.float32)
    return dict(c, init=(c["init"][0], xf))


def test_pinhole_start_behind_the_near_plane_is_refused():
    c = _behind(vc.subset(vc.case("pinhole"), np.arange(5)), 1)
    got, want = _gpu(c, 8), vc.restate(c, np.float64, 8)
    assert np.array_equal(got["info"][:, 3].astype(int) & vc.REFUSED, [0, 4, 0, 0, 0])
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32))
    assert not got["ja"][1].any() and np.array_equal(got["xf"][1], np.eye(4, dtype=np.float32)) and not got["info"][1, :3].any()
    assert not got["residual"][1].any() and all(np.isfinite(got[k]).all() for k in got)


def _crossing_case():
    """Pinhole views whose detections are the hand's, magnified 4 x about the principal point: the picture of a hand four times
    as near.  The Gauss-Newton step d z = -(k - 1) z takes the hand through the cameras: the first trial lies behind the near
    plane of both views."""
    c = vc.subset(vc.case("pinhole"), np.arange(5))
    centre = c["table"][c["cam_rows"]][:, :, None, 2:4]
    return dict(c, window=centre + 4.0 * (c["window"] - centre), init=(c["init"][0], c["init"][1].copy()))


def test_step_across_the_near_plane_is_rejected():
    """The first trial crosses the near plane (the float64 restatement's cost there is +inf): max_iters = 1 returns the start's
    bits with its rms and worst, AT_MAX_ITERS; max_iters = 12 ends finite, below the start's cost, with the restatement's
    status, and no landmark of the returned pose in front of a near plane."""
    c = _crossing_case()
    n = len(c["mirror"])
    trace = []
    want1 = vc.restate(c, np.float64, 1, trace=trace)
    assert np.all(np.isinf(trace[0]["trial_cost"])) and not trace[0]["accept"].any()
    one = _gpu(c, 1)
    assert np.array_equal(_bits(one["ja"]), _bits(c["init"][0])) and np.array_equal(_bits(one["xf"]), _bits(c["init"][1]))
    assert np.array_equal(one["info"][:, 2:], np.tile(np.float32([1, _native.UT_FIT_AT_MAX_ITERS]), (n, 1)))
    tol = vc.bounds_from(vc.float32_distance(c, want1))
    off = float(np.abs(one["info"][:, :2] - want1["info"][:, :2]).max())
    print(f"start's rms / worst after a rejected trial: off by {off:.1e} px (bound {tol['px']:.1e}; rms up to {want1['info'][:, 0].max():.0f} px)")
    assert off <= tol["px"]
    assert np.abs(one["residual"] - want1["residual"]).max() <= tol["px"] + tol["kp"] * _px_per_mm(c)
    want = vc.restate(c, np.float64, 12)
    got = _gpu(c, 12)
    assert all(np.isfinite(got[k]).all() for k in got)
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32)) and np.all(got["info"][:, 2] > 1)
    assert np.all(got["info"][:, 0] < one["info"][:, 0])
    tab = c["table"][c["cam_rows"]]
    ez = np.stack([tc.project(tab[:, v, None, :], vc.landmarks(c, got), tc.PINHOLE)[1] for v in range(2)], 1)
    assert ez.min() >= tc.NEAR_Z


def test_cam_rows_out_of_range_is_the_index_check():
    c = vc.subset(vc.case("two_views"), np.arange(5))
    rows = c["cam_rows"].copy()
    rows[2, 1] = len(c["table"])
    out = (torch.full((5, 22), 7.0, device=DEV), torch.full((5, 4, 4), 7.0, device=DEV))
    info, res = torch.full((5, 4), 7.0, device=DEV), torch.full((5, 2, 21), 7.0, device=DEV)
    with pytest.raises(IndexError):
        _native.fit_pose_views(_blob(c["hm"]), _t(c["window"], torch.float64), _t(rows, torch.int32), _t(c["table"], torch.float64),
                               _t(c["init"][0]), _t(c["init"][1]), _t(c["weights"]), mirror=_t(c["mirror"], torch.int64), out=out,
                               info=info, residual=res)
    torch.cuda.synchronize()
    for t in out + (info, res):
        assert bool((t[2] == 7.0).all()) and bool((t[[0, 1, 3, 4]] != 7.0).any())
    ok = _gpu(c, 32)
    assert np.array_equal(_bits(out[0].cpu().numpy()[[0, 1, 3, 4]]), _bits(ok["ja"][[0, 1, 3, 4]]))
    with pytest.raises(ValueError):
        _native.fit_pose_views(_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64),
                               None, None)


def test_capturable_with_deferred_checks():
    """With an engine in deferred-check mode the launch synchronises nothing: captured in a graph and replayed it gives the bits
    of the eager run, and a cam_rows entry out of range raises from poll_status, not from the call."""
    c = vc.case("ragged")
    blob, win, rows, table = _blob(c["hm"]), _t(c["window"], torch.float64), _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64)
    ja0, xf0, w, mirror = _t(c["init"][0]), _t(c["init"][1]), _t(c["weights"]), _t(c["mirror"], torch.int64)

    def buffers():
        return dict(ja=torch.zeros(74, 22, device=DEV), xf=torch.zeros(74, 4, 4, device=DEV), info=torch.zeros(74, 4, device=DEV),
                    res=torch.zeros(74, 3, 21, device=DEV))

    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            def fit(b, r):
                _native.fit_pose_views(blob, win, r, table, ja0, xf0, w, mirror=mirror, out=(b["ja"], b["xf"]), info=b["info"],
                                       residual=b["res"], engine=eng)

            eager, replayed = buffers(), buffers()
            fit(eager, rows)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fit(replayed, rows)
            graph.replay()
            torch.cuda.synchronize()
            eng.poll_status()
            bad = rows.clone()
            bad[5, 0] = table.shape[0]
            fit(buffers(), bad)                       # no error here ...
            torch.cuda.synchronize()
            with pytest.raises(IndexError):
                eng.poll_status()                     # ... but here
    finally:
        eng.close()
    for name in eager:
        assert torch.equal(eager[name].view(torch.int32), replayed[name].view(torch.int32)), name
    assert bool((eager["info"][:, 2] >= 1).all())


def test_residual_is_the_projection_of_fk_of_the_returned_pose():
    """residual against ut_project_points of ut_fk of the returned pose minus the windows.  Both project the fp32 landmarks of
    ut_fk's arithmetic in fp64; what may differ is one fp32 ulp of a landmark coordinate - the kernel holds the wrist in
    target units and divides by t_scale on the way out - times the cameras' px per mm, per coordinate, and the rounding of the
    distance itself to fp32."""
    c = vc.case("ragged")
    got = _gpu(c, 32)
    kp = _native.fk_stateless(_blob(c["hm"]), _t(got["ja"]), _t(got["xf"]), _t(c["mirror"], torch.int64))
    size = vc.golden()["size"]
    win = _native.project_points(kp, _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64), size[0], size[1])[0].cpu().numpy()
    used = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64).used
    dist = np.where(used, np.linalg.norm(win - np.where(used[..., None], c["window"], 0.0), axis=-1), 0.0)
    ulp = 2.0 ** -23 * float(np.abs(kp.cpu().numpy()).max())
    bound = 3 * ulp * _px_per_mm(c) + 2.0 ** -23 * float(dist.max())
    d = float(np.abs(got["residual"] - dist).max())
    print(f"residual vs project(fk(pose)): {d:.2e} px (bound {bound:.2e}), residuals up to {dist.max():.2e} px")
    assert not got["residual"][~used].any() and d <= bound


# ----------------------------------------------------------------------------- 4. the Python layers
def _frame_of(i):
    z = np.load(tc.GOLDEN + "/projection_rec00.npz")
    return int(z["frame"][z["case_frame"]][i])


def test_refine_hand_pose_in_views_with_one_camera():
    """One camera, hands 3 (left) and 40: tracker.refine_hand_pose_in_views returns the float64 restatement's pose within the
    bound rule, info [4] and residual [1,21] with it."""
    g, c = vc.golden(), vc.full_case("one")
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    for i in (3, 40):
        cams = pipeline.cameras_for_frame(lab, _frame_of(i))
        cam = [cams[int(g["best"][i, 0])]]
        one = vc.subset(c, [i])
        one.update(table=tracker._native_camera_table(cam, "test"), cam_rows=np.zeros((1, 1), np.int32))
        init = tracker.SingleHandPose(joint_angles=one["init"][0][0], wrist_xform=one["init"][1][0], hand_confidence=1.0)
        pose, info, residual = tracker.refine_hand_pose_in_views(model, cam, one["window"][0], int(g["hand"][i]), init, one["weights"][0])
        want = vc.restate(one, np.float64, 32)
        got = dict(ja=pose.joint_angles[None], xf=pose.wrist_xform[None], info=info[None])
        d, tol = vc.distance(one, got, want), vc.bounds_from(vc.float32_distance(one, want, 32))
        _show(f"refine_hand_pose_in_views, one camera, hand {i}", d, tol)
        assert pose.hand_confidence == 1.0 and info.shape == (4,) and residual.shape == (1, 21) and int(info[3]) == _native.UT_FIT_CONVERGED
        assert vc.within(d, tol)


def test_hand_pose_from_window_keypoints_refined_in_the_views():
    """The ragged noisy case (1 px, the second view missing 12 landmarks), hands 0, 1 and 2: refine_in_views=True returns a pose
    whose reprojection cost over all detections is at most the unrefined chain's, and the float64 restatement's from the
    chain's pose within the bound rule; refine_in_views=False is the default call and the chain alone, bit for bit."""
    g, c = vc.golden(), vc.noisy_ragged()
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    for i in (0, 1, 2):
        cams = [pipeline.cameras_for_frame(lab, _frame_of(i))[int(k)] for k in g["seeing"][i]]
        win, w, h = c["window"][i], c["weights"][i], int(g["hand"][i])
        plain, info_plain = tracker.hand_pose_from_window_keypoints(model, cams, win, h, weights=w, use_information=True)
        off, info_off = tracker.hand_pose_from_window_keypoints(model, cams, win, h, weights=w, use_information=True, refine_in_views=False)
        alone = tracker._chain_pose_from_window_keypoints(model, cams, win, h, w, None, True)[0]
        for other in (off, alone):
            assert np.array_equal(_bits(plain.joint_angles), _bits(other.joint_angles)) and np.array_equal(_bits(plain.wrist_xform), _bits(other.wrist_xform))
        assert np.array_equal(_bits(info_plain), _bits(info_off))
        fine, info_fine = tracker.hand_pose_from_window_keypoints(model, cams, win, h, weights=w, use_information=True, refine_in_views=True)
        assert np.array_equal(_bits(info_fine), _bits(info_plain))
        one = vc.subset(c, [i])
        one.update(table=tracker._native_camera_table(cams, "test"), cam_rows=np.arange(2, dtype=np.int32)[None],
                   init=(plain.joint_angles[None].astype(np.float32), plain.wrist_xform[None].astype(np.float32)))
        vw = vc.Views(one["window"], one["cam_rows"], one["table"], one["weights"], np.float64)
        cost = lambda p: float(vw.cost(vc.landmarks(one, dict(ja=p.joint_angles[None], xf=p.wrist_xform[None])), np.arange(1), np.float64)[0][0])
        want = vc.restate(one, np.float64, 32)
        got = dict(ja=fine.joint_angles[None], xf=fine.wrist_xform[None], info=want["info"])
        d, tol = vc.distance(one, got, want), vc.bounds_from(vc.float32_distance(one, want, 32))
        print(f"hand {i}: reprojection cost over all detections, chain {cost(plain):.1f} -> refined {cost(fine):.1f} px^2")
        _show(f"   against the restatement from the chain's pose", d, tol)
        assert cost(fine) <= cost(plain) and vc.within(d, tol)


def test_fit_landmarks_views_and_fit_keypoints_in_views_batch():
    """hand.fit_landmarks_views with leading dims [2,37] from the CPU, and pipeline.fit_keypoints_in_views on the device, give the
    bits of _native.fit_pose_views on the 74 hands."""
    c = vc.full_case("two")
    base = _gpu(c, 32)
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)) if dt is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    ja, xf, info, res = hand.fit_landmarks_views(model, t(c["window"]).reshape(2, 37, 2, 21, 2), t(c["cam_rows"]).reshape(2, 37, 2), t(c["table"]),
                                                 (t(c["init"][0]).reshape(2, 37, 22), t(c["init"][1]).reshape(2, 37, 4, 4)),
                                                 weights=t(c["weights"]).reshape(2, 37, 2, 21), mirror=t(c["mirror"]).reshape(2, 37), with_residual=True)
    assert ja.shape == (2, 37, 22) and xf.shape == (2, 37, 4, 4) and info.shape == (2, 37, 4) and res.shape == (2, 37, 2, 21) and ja.device.type == "cpu"
    got = dict(ja=ja.reshape(74, 22).numpy(), xf=xf.reshape(74, 4, 4).numpy(), info=info.reshape(74, 4).numpy(), residual=res.reshape(74, 2, 21).numpy())
    assert _same_bits(got, base)
    with pytest.raises(ValueError):
        hand.fit_landmarks_views(model, t(c["window"]), t(c["cam_rows"]), t(c["table"]), None)
    out = pipeline.fit_keypoints_in_views(_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["table"], torch.float64), _t(c["cam_rows"], torch.int32),
                                          _t(c["init"][0]), _t(c["init"][1]), weights=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64),
                                          with_residual=True)
    assert _same_bits(dict(zip(("ja", "xf", "info", "residual"), (o.cpu().numpy() for o in out))), base)
