"""GPU tests of the robust pose fit in the views (csrc/fit_views_robust.hip through ut_fit_pose_views_robust,
hand.fit_landmarks_views, pipeline.fit_keypoints_in_views and tracker.refine_hand_pose_in_views) against the float64 / float32
numpy restatement of tests/robust_cases.py, which tests/test_robust_host.py checks.  The shapes are the 74 golden hands and
slices of 1 and 5.

The sharp checks are one-step checks: bounds by robust_cases.bounds_from (views_cases.bounds_from on the robust restatement, and
for `inlier` 4 x the float32 restatements' distance from the float64 psi at their returned poses, at least 2^-24), computed here from the restatements,
never from the kernel's output, and printed.  Full fits are judged on the hands the restatements themselves select
(robust_cases.selected), by distance to the truth, with no iteration rule and no pose-to-pose comparison: on contaminated data
the cost has several basins and valleys along depth, where two correct solvers end apart.  Measured figures: DESIGN.md, "Pose
from keypoints in the views, robust"."""
import numpy as np
import pytest
import torch

import fit_cases as fc
import robust_cases as rc
import step_cases as st
import views_cases as vc
from absolutetrack_amd import _native, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("ja", "xf", "info", "residual", "inlier")


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(*(hm[k] for k in st.FIELDS))).reshape(-1, 321)


def _inputs(c):
    return (_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64),
            _t(c["init"][0]), _t(c["init"][1]), None if c["weights"] is None else _t(c["weights"]),
            None if c["limits"] is None else _t(c["limits"]), _t(c["mirror"], torch.int64))


def _gpu(c, max_iters, **kw):
    """The case on the GPU -> numpy dict(ja [n,22], xf [n,4,4], info [n,4], residual [n,V,21], inlier [n,V,21])."""
    n = len(c["mirror"])
    out = _native.fit_pose_views_robust(*_inputs(c), t_scale=c["t_scale"], max_iters=max_iters, loss=c["loss"], loss_scale=c["loss_scale"],
                                        residual=True, inlier=True, **kw)
    torch.cuda.synchronize()
    got = dict(zip(OUT, (o.cpu().numpy() for o in out)))
    got["xf"] = got["xf"].reshape(n, 4, 4)
    return got


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, keys=OUT):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _padded(c, slots):
    """The case on max_views = len(slots) + unused slots: view j of the case in slot slots[j], -1 rows with NaN windows and NaN
    weights elsewhere.  slots (0, 1) of 3: a trailing unused view; (0, 2): a -1 hole."""
    n, v = c["cam_rows"].shape
    total = 3
    win, rows, w = np.full((n, total, 21, 2), np.nan), np.full((n, total), -1, np.int32), np.full((n, total, 21), np.nan, np.float32)
    for j, s in enumerate(slots):
        win[:, s], rows[:, s], w[:, s] = c["window"][:, j], c["cam_rows"][:, j], c["weights"][:, j]
    return dict(c, window=win, cam_rows=rows, weights=w)


def _show(what, d, tol):
    print(f"{what}: angles {d['ang']:.2e} (bound {tol['ang']:.2e}) rad, landmarks {d['kp']:.2e} ({tol['kp']:.2e}) mm, rms / worst "
          f"{d['px']:.2e} ({tol['px']:.2e}) px, inlier {d['inlier']:.2e} ({tol['inlier']:.2e})")


def _px_per_mm(c):
    vw = rc.views_of(c)
    jacs = vw.blocks(c["truth"], np.arange(len(c["truth"])))[6]
    return float(max(np.linalg.norm(j, axis=(-2, -1)).max() for j in jacs))


# ----------------------------------------------------------------------------- 1. one step
ONE_STEP = [(name, loss, rc.SCALE_PX, False) for loss in rc.ROBUST for name in rc.STEP_CASES] + \
           [("two_views", loss, scale, True) for loss in rc.ROBUST for scale in (1.0, 1e4)]


@pytest.mark.parametrize("name,loss,scale,dirty", ONE_STEP)
def test_one_step(name, loss, scale, dirty):
    """max_iters = 1 from the +-0.2 rad / +-15 mm starts of the 74 golden hands, where nearly every residual lies in the robust
    regime: the 20 angles, the wrist, rms and worst against the float64 restatement's one step, landmarks through the float64
    forward function of both, `inlier` against the float64 psi at the returned pose; one iteration, the restatement's status;
    the residuals of the returned pose.  dirty: two views with 2 detections each displaced by 40 px, at a scale of 1 px and of
    1e4 px (where the loss is the squared one to 1e-5).
    `inlier` is held against the float64 psi at the pose the kernel itself returned (robust_cases.psi_at: float64 forward function
    and projection), as the bound is the float32 restatements' distance from the float64 psi at theirs: that measures the output.
    How far the kernel's pose lies from the float64 restatement's is what angles and landmarks measure; through it the two psi differ
    by up to 3.3e-4 on the worst-conditioned hand of mixed / geman_mcclure, which no bound here is about."""
    c = rc.step_case(name, loss, scale, dirty)
    n = len(c["mirror"])
    trace = []
    want = rc.restate(c, np.float64, 1, trace=trace)
    got = _gpu(c, 1)
    d, tol = rc.distance(c, got, want), rc.bounds_from(rc.float32_distance(c, want))
    _show(f"one step, {name}{' dirty' if dirty else ''}, {loss} at {scale:g} px ({int(trace[0]['accept'].sum())} of {n} accepted)", d, tol)
    assert np.array_equal(got["info"][:, 2], np.ones(n, np.float32))
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32))
    assert np.array_equal(_bits(got["ja"][:, 20:]), _bits(c["init"][0][:, 20:]))
    assert st.within(d, tol), (d, tol)
    used = rc.views_of(c).used
    assert not got["residual"][~used].any() and not got["inlier"][~used].any()
    assert np.all(got["inlier"][used] > 0) and got["inlier"].max() <= 1
    assert np.abs(got["residual"] - want["residual"]).max() <= tol["px"] + tol["kp"] * _px_per_mm(c)


# ----------------------------------------------------------------------------- 2. the squared loss
@pytest.mark.parametrize("name", ["two_views", "ragged"])
def test_squared_loss_is_fit_pose_views(name):
    """UT_LOSS_SQUARED gives the bits of ut_fit_pose_views - pose, info and residual, full fits -, with `inlier` (the squared
    instantiation of the robust kernels, which knows the refusals) and without (fit_views.hip's kernels themselves); inlier is
    the mask of used observations.  The scale is not read: NaN."""
    c = rc.step_case(name, "squared", float("nan"))
    plain = _native.fit_pose_views(*_inputs(c), t_scale=c["t_scale"], max_iters=32, residual=True)
    no_inlier = _native.fit_pose_views_robust(*_inputs(c), t_scale=c["t_scale"], max_iters=32, loss="squared", loss_scale=float("nan"),
                                              residual=True)
    torch.cuda.synchronize()
    assert len(no_inlier) == 4
    want = dict(zip(OUT, (o.cpu().numpy() for o in plain)))
    got = _gpu(c, 32)
    assert _same_bits(got, want, OUT[:4])
    assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())) for a, b in zip(plain, no_inlier))
    assert np.all(got["info"][:, 3] != _native.UT_FIT_REFUSED)
    assert np.array_equal(got["inlier"], rc.views_of(c).used.astype(np.float32))


# ----------------------------------------------------------------------------- 3. full fits on the selected hands
def test_full_fits_on_the_selected_hands():
    """Two views, 2 detections per view displaced by 40 px, tracking starts, Geman-McClure at 3 px, max_iters = 32, on the hands
    the host purpose check selects (70 of 74): every pose UT_FIT_CONVERGED; landmarks within max(KP_TOL_MM, 4 x the worse float32
    restatement's error to the truth over the same hands) of the truth; inlier < 0.5 exactly on the displaced detections."""
    sel, runs, errs = rc.selected()
    c = rc.subset(rc.tracked_case("two", "geman_mcclure"), sel)
    got = _gpu(c, 32)
    err = np.linalg.norm(vc.landmarks(c, got) - c["truth"], axis=-1).max(1)
    bound = max(st.KP_TOL_MM, st.FLOAT32_FACTOR * float(errs[:2, sel].max()))
    its = got["info"][:, 2]
    print(f"{len(sel)} selected hands: GPU worst landmark {err.max():.2e} mm (bound {bound:.2e}; float32 restatements {errs[:2, sel].max():.2e}, float64 "
          f"{errs[2, sel].max():.2e}), iterations mean {its.mean():.1f} max {int(its.max())} (float64 restatement mean "
          f"{runs[2]['info'][sel, 2].mean():.1f} max {int(runs[2]['info'][sel, 2].max())}), robust rms up to {got['info'][:, 0].max():.2e} px")
    assert len(sel) >= 56
    assert np.array_equal(got["info"][:, 3], np.full(len(sel), _native.UT_FIT_CONVERGED, np.float32))
    assert err.max() <= bound
    used = rc.views_of(c).used
    assert np.array_equal((got["inlier"] < 0.5) & used, c["displaced"]) and not got["inlier"][~used].any()


# ----------------------------------------------------------------------------- 4. where basins rule
def test_sanity_where_basins_rule():
    """The best view alone, 4 of its detections displaced by 40 px, Huber at 3 px, tracking starts, max_iters = 32: one view
    leaves depth to the hand's size and 4 outliers pull with Huber's full linear force, so where a fit ends is the cost's
    business.  Every output is finite, every status converged or at-max-iters, and the robust cost of the returned pose,
    evaluated in float64 on the host, exceeds the start's by at most a rounding allowance: fc.FLAT_TOL x the start's cost (the
    fit stops at the accepted state's cost in fp32) unless the float32 restatements' own excess is larger - then 4 x theirs."""
    c = rc.tracked_case("one", "huber", 4)
    start = dict(ja=c["init"][0], xf=c["init"][1])
    cost0 = rc.robust_cost(c, start)
    excess = lambda r: float(((rc.robust_cost(c, r) - cost0) / cost0).max())
    own = max(excess(rc.restate(c, np.float32, 32, s)) for s in st.SOLVERS)
    allowance = fc.FLAT_TOL if own <= fc.FLAT_TOL else st.FLOAT32_FACTOR * own
    got = _gpu(c, 32)
    status = got["info"][:, 3].astype(int)
    print(f"best view, 4 outliers, Huber: relative excess of the returned cost over the start's {excess(got):.2e} (allowance {allowance:.2e}: "
          f"{'FLAT_TOL' if own <= fc.FLAT_TOL else '4 x the float32 restatements'}, whose own excess is {own:.2e}); converged "
          f"{int((status == 1).sum())}, at max_iters {int((status == 2).sum())} of 74")
    assert all(np.isfinite(got[k]).all() for k in OUT)
    assert np.all((status == _native.UT_FIT_CONVERGED) | (status == _native.UT_FIT_AT_MAX_ITERS))
    assert excess(got) <= allowance


# ----------------------------------------------------------------------------- 5. shapes and plumbing
@pytest.mark.parametrize("loss", rc.ROBUST)
def test_batches_and_padding_leave_the_bits(loss):
    """A pose alone (a workgroup with one live wave), in a batch of 5 and in the batch of 74 gives the same bits; so does
    max_views = 3 with a trailing unused view or with a -1 hole between the two views."""
    c = rc.tracked_case("two", loss)
    whole = _gpu(c, 32)
    for sel in (np.array([41]), np.arange(6, 11)):
        assert _same_bits(_gpu(rc.subset(c, sel), 32), {k: v[sel] for k, v in whole.items()}), (loss, sel)
    for slots in ((0, 1), (0, 2)):
        padded = _gpu(_padded(c, slots), 32)
        other = ({0, 1, 2} - set(slots)).pop()
        assert not padded["residual"][:, other].any() and not padded["inlier"][:, other].any()
        for k in ("residual", "inlier"):
            padded[k] = padded[k][:, list(slots)]
        assert _same_bits(padded, whole), (loss, slots)


def _decision_case(loss):
    c = rc.subset(rc.step_case("two_views", loss), np.arange(8))
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


@pytest.mark.parametrize("loss", rc.ROBUST)
def test_refusals_keep_the_start_and_nan_at_weight_0_changes_nothing(loss):
    c = _decision_case(loss)
    got, want = _gpu(c, 32), rc.restate(c, np.float64, 32)
    assert np.array_equal(got["info"][:, 3].astype(int) & vc.REFUSED, [0, 4, 4, 4, 4, 0, 0, 0])
    assert np.array_equal(got["info"][:, 3].astype(int) & vc.REFUSED, want["info"][:, 3].astype(int) & vc.REFUSED)
    assert all(np.isfinite(got[k]).all() for k in OUT)
    assert np.array_equal(_bits(got["ja"][1:5]), _bits(c["init"][0][1:5])) and np.array_equal(_bits(got["xf"][1:5]), _bits(c["init"][1][1:5]))
    assert not got["info"][1:5, :3].any() and not got["residual"][1:5].any() and not got["inlier"][1:5].any()
    assert not got["inlier"][5, 1].any() and got["inlier"][0, 1, 4] == 0 and np.all(got["inlier"][5, 0] > 0)
    garbage = c["window"].copy()
    garbage[0, 1, 4] = 123.5
    assert _same_bits(got, _gpu(dict(c, window=garbage), 32))


def test_pinhole_start_behind_the_near_plane_is_refused_with_inlier_0():
    c = rc.subset(rc.step_case("pinhole", "huber"), np.arange(5))
    cam = c["table"][c["cam_rows"][1, 0]]
    axis = cam[4:13].reshape(3, 3)[:, 2]
    xf = c["init"][1].copy()
    xf[1, :3, 3] -= (2 * (axis @ (c["truth"][1].mean(0) - cam[13:16])) * axis).astype(np.float32)
    got = _gpu(dict(c, init=(c["init"][0], xf)), 8)
    assert np.array_equal(got["info"][:, 3].astype(int) & vc.REFUSED, [0, 4, 0, 0, 0])
    assert not got["ja"][1].any() and np.array_equal(got["xf"][1], np.eye(4, dtype=np.float32)) and not got["info"][1, :3].any()
    assert not got["residual"][1].any() and not got["inlier"][1].any() and all(np.isfinite(got[k]).all() for k in OUT)


def test_cam_rows_out_of_range_is_the_index_check():
    """An entry outside [-1, n_rows) writes nothing for its pose, inlier included, and raises from the call with the checks
    synchronous, from poll_status with an engine in deferred-check mode."""
    c = rc.subset(rc.tracked_case("two", "geman_mcclure"), np.arange(5))
    rows = c["cam_rows"].copy()
    rows[2, 1] = len(c["table"])
    bad = dict(c, cam_rows=rows)

    def buffers():
        return dict(out=(torch.full((5, 22), 7.0, device=DEV), torch.full((5, 4, 4), 7.0, device=DEV)), info=torch.full((5, 4), 7.0, device=DEV),
                    residual=torch.full((5, 2, 21), 7.0, device=DEV), inlier=torch.full((5, 2, 21), 7.0, device=DEV))

    def untouched_pose_2(b):
        for t in b["out"] + (b["info"], b["residual"], b["inlier"]):
            assert bool((t[2] == 7.0).all()) and bool((t[[0, 1, 3, 4]] != 7.0).any())

    kw = dict(t_scale=1.0, max_iters=32, loss=c["loss"], loss_scale=c["loss_scale"])
    b = buffers()
    with pytest.raises(IndexError):
        _native.fit_pose_views_robust(*_inputs(bad), **kw, **b)
    torch.cuda.synchronize()
    untouched_pose_2(b)
    ok = _gpu(c, 32)
    assert np.array_equal(_bits(b["out"][0].cpu().numpy()[[0, 1, 3, 4]]), _bits(ok["ja"][[0, 1, 3, 4]]))
    assert np.array_equal(_bits(b["inlier"].cpu().numpy()[[0, 1, 3, 4]]), _bits(ok["inlier"][[0, 1, 3, 4]]))
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            b = buffers()
            _native.fit_pose_views_robust(*_inputs(bad), **kw, **b, engine=eng)      # no error here ...
            torch.cuda.synchronize()
            with pytest.raises(IndexError):
                eng.poll_status()                                                     # ... but here
            untouched_pose_2(b)
            good = buffers()
            _native.fit_pose_views_robust(*_inputs(c), **kw, **good, engine=eng)
            torch.cuda.synchronize()
            eng.poll_status()
    finally:
        eng.close()
    assert np.array_equal(_bits(good["inlier"].cpu().numpy()), _bits(ok["inlier"]))


@pytest.mark.parametrize("loss", rc.ROBUST)
def test_inlier_is_psi_of_the_residual(loss):
    """inlier == psi((residual / c)^2): the kernel forms both from one fp64 squared distance, `residual` is its root rounded to
    fp32 (2^-24 relative, which psi at most doubles: 2^-22 of a value <= 1 for the square and Geman-McClure's power) and
    `inlier` is rounded once more (2^-24)."""
    c = rc.tracked_case("two", loss)
    got = _gpu(c, 32)
    used = rc.views_of(c).used & ~(got["info"][:, 3].astype(int) & vc.REFUSED != 0)[:, None, None]
    want = np.where(used, rc.psi(loss, got["residual"].astype(np.float64) ** 2, c["loss_scale"]), 0.0)
    d = float(np.abs(got["inlier"] - want).max())
    print(f"{loss}: inlier vs psi of the residual {d:.2e} (bound {5 * 2.0 ** -24:.2e}); inlier min {got['inlier'][used].min():.2e}")
    assert d <= 5 * 2.0 ** -24 and got["inlier"][used].min() < 0.5 < got["inlier"][used].max()


# ----------------------------------------------------------------------------- 6. the Python layers
def _frame_of(i):
    import triangulate_cases as tc
    z = np.load(tc.GOLDEN + "/projection_rec00.npz")
    return int(z["frame"][z["case_frame"]][i])


def test_refine_hand_pose_in_views_is_the_native_entry():
    """tracker.refine_hand_pose_in_views(..., loss="geman_mcclure") on two contaminated hands, one left and one right: the bits of
    _native.fit_pose_views_robust on the same arrays, and a fourth item, the inliers."""
    g, c = vc.golden(), rc.tracked_case("two", "geman_mcclure")
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    hands = (3, 40)
    assert {int(g["hand"][i]) for i in hands} == {0, 1}
    for i in hands:
        cams = [pipeline.cameras_for_frame(lab, _frame_of(i))[int(k)] for k in g["seeing"][i]]
        table = tracker._native_camera_table(cams, "test")
        win, w = c["window"][i], c["weights"][i]
        init = tracker.SingleHandPose(joint_angles=c["init"][0][i], wrist_xform=c["init"][1][i], hand_confidence=1.0)
        pose, info, residual, inlier = tracker.refine_hand_pose_in_views(model, cams, win, int(g["hand"][i]), init, w, loss="geman_mcclure",
                                                                         loss_scale=rc.SCALE_PX)
        ja, xf, ninfo, nres, ninl = _native.fit_pose_views_robust(
            hand.device_blob(model, torch.device(DEV)), _t(win[None], torch.float64), torch.arange(2, dtype=torch.int32, device=DEV)[None],
            _t(table, torch.float64), _t(c["init"][0][i][None]), _t(c["init"][1][i][None]), _t(w[None]), None,
            _t(np.array([1 if int(g["hand"][i]) == tracker.RIGHT_HAND_INDEX else 0]), torch.int64), loss="geman_mcclure",
            loss_scale=rc.SCALE_PX, residual=True, inlier=True)
        for a, b in ((pose.joint_angles, ja[0]), (pose.wrist_xform, xf[0]), (info, ninfo[0]), (residual, nres[0]), (inlier, ninl[0])):
            assert np.array_equal(_bits(a), _bits(b.cpu().numpy()))
        assert inlier.shape == (2, 21) and np.array_equal(inlier < 0.5, c["displaced"][i]) and int(info[3]) == _native.UT_FIT_CONVERGED
        plain = tracker.refine_hand_pose_in_views(model, cams, win, int(g["hand"][i]), init, w)
        assert len(plain) == 3


def test_fit_landmarks_views_defaults_are_the_plain_fit():
    """hand.fit_landmarks_views and pipeline.fit_keypoints_in_views: the defaults give the bits of _native.fit_pose_views;
    loss="squared" with return_inliers adds the used mask; a robust loss gives the bits of _native.fit_pose_views_robust."""
    c = rc.tracked_case("two", "huber")
    n = len(c["mirror"])
    base = _native.fit_pose_views(*_inputs(c), max_iters=32, residual=True)
    robust = _gpu(c, 32)
    torch.cuda.synchronize()
    base = [b.cpu().numpy() for b in base]
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (model, t(c["window"]), t(c["cam_rows"]), t(c["table"]), (t(c["init"][0]), t(c["init"][1])))
    kw = dict(weights=t(c["weights"]), mirror=t(c["mirror"]))
    plain = hand.fit_landmarks_views(*args, **kw, with_residual=True)
    assert len(plain) == 4 and all(np.array_equal(_bits(a.numpy()), _bits(b)) for a, b in zip(plain, base))
    assert len(hand.fit_landmarks_views(*args, **kw)) == 3
    masked = hand.fit_landmarks_views(*args, **kw, with_residual=True, return_inliers=True)
    assert len(masked) == 5 and all(np.array_equal(_bits(a.numpy()), _bits(b)) for a, b in zip(masked, base))
    assert np.array_equal(masked[4].numpy(), rc.views_of(c).used.astype(np.float32))
    fine = hand.fit_landmarks_views(*args, **kw, with_residual=True, loss="huber", loss_scale=c["loss_scale"], return_inliers=True)
    assert len(fine) == 5 and all(np.array_equal(_bits(a.numpy().reshape(robust[k].shape)), _bits(robust[k])) for a, k in zip(fine, OUT))
    out = pipeline.fit_keypoints_in_views(_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["table"], torch.float64), _t(c["cam_rows"], torch.int32),
                                          _t(c["init"][0]), _t(c["init"][1]), weights=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64),
                                          with_residual=True, loss="huber", loss_scale=c["loss_scale"], with_inliers=True)
    assert all(np.array_equal(_bits(a.cpu().numpy().reshape(robust[k].shape)), _bits(robust[k])) for a, k in zip(out, OUT))
    out = pipeline.fit_keypoints_in_views(_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["table"], torch.float64), _t(c["cam_rows"], torch.int32),
                                          _t(c["init"][0]), _t(c["init"][1]), weights=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64),
                                          with_residual=True)
    assert len(out) == 4 and all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(out, base)) and n == 74
