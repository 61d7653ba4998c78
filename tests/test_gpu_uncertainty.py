"""GPU tests of the uncertainty of a pose fitted in the views (csrc/pose_info_views.hip through ut_pose_information_views,
hand.pose_uncertainty_views, pipeline.fit_keypoints_in_views and tracker.refine_hand_pose_in_views) against the float64 /
float32 numpy restatement of tests/uncertainty_cases.py, which tests/test_uncertainty_host.py checks.  The shapes are the 74
golden hands (19 workgroups) and slices of 1 and 5.

Bounds by uncertainty_cases.bounds_from - DESIGN's rule for one step against float64: step_cases.FLOAT32_FACTOR x the worst
distance of the two float32 restatements from float64 on the case, computed here from the restatements, never from the
kernel's output, and printed next to the kernel's distance.  Measured figures: DESIGN.md, "Uncertainty of a pose fitted in the
views"."""
import numpy as np
import pytest
import torch

import robust_cases as rc
import step_cases as st
import uncertainty_cases as uc
import views_cases as vc
from absolutetrack_amd import _native, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("pose_info", "pivot", "param_sigma", "landmark_cov", "info")


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(*(hm[k] for k in st.FIELDS))).reshape(-1, 321)


def _inputs(c):
    """(positional arguments, keywords) of _native.pose_information_views for a case."""
    return ((_blob(c["hm"]), _t(c["ja"]), _t(c["xf"]), _t(c["window"], torch.float64), _t(c["cam_rows"], torch.int32),
             _t(c["table"], torch.float64)),
            dict(weights=None if c["weights"] is None else _t(c["weights"]),
                 angle_sigma=None if c["angle_sigma"] is None else _t(c["angle_sigma"]), mirror=_t(c["mirror"], torch.int64),
                 t_scale=c["t_scale"], loss=c["loss"], loss_scale=c["loss_scale"]))


def _raw(c, **kw):
    """The case on the GPU: the five packed outputs as numpy arrays."""
    args, base = _inputs(c)
    out = _native.pose_information_views(*args, **dict(base, **kw))
    torch.cuda.synchronize()
    return dict(zip(OUT, (o.cpu().numpy() for o in out)))


def _unpacked(raw):
    return dict(raw, pose_info=uc.untril(raw["pose_info"]), landmark_cov=uc.uncov(raw["landmark_cov"]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in OUT)


def _show(what, d, d32, tol):
    print(f"{what}: " + ", ".join(f"{k} GPU {d[k]:.2e} float32 {d32[k]:.2e} bound {tol[k]:.2e}" for k in uc.QUANTITIES))


def _padded(c, slots, total=3):
    """View j of the case in slot slots[j] of `total`: -1 rows with NaN windows and NaN weights elsewhere."""
    n = len(c["cam_rows"])
    win, rows, w = np.full((n, total, 21, 2), np.nan), np.full((n, total), -1, np.int32), np.full((n, total, 21), np.nan, np.float32)
    for j, s in enumerate(slots):
        win[:, s], rows[:, s], w[:, s] = c["window"][:, j], c["cam_rows"][:, j], c["weights"][:, j]
    return dict(c, window=win, cam_rows=rows, weights=w)


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("name", uc.REGULAR + uc.ROBUST + ("free_finger_prior",))
def test_against_float64(name):
    """Every regular case - max_views 1 (best_view), 2, 3 with a -1 hole and NaN windows at weight 0 (ragged); n_models 1 and n
    (mixed); both camera kinds; metres; mirrored and unmirrored hands in every batch; Huber and Geman-McClure on displaced
    detections; the prior: the four quantities, and the rms and the smallest pivot of info, within the rule's bounds of float64;
    UT_COV_OK on every pose; info[1] is the largest landmark sigma of the covariances written."""
    c, want = uc.case(name), uc.oracle(name)
    assert set(c["mirror"]) == {0, 1} and np.all(want["info"][:, 3] == uc.OK)
    raw = _raw(c)
    got = _unpacked(raw)
    d, d32 = uc.distance(c, got, want), uc.float32_distance(name)
    tol = uc.bounds_from(d32)
    _show(name, d, d32, tol)
    assert np.array_equal(got["info"][:, 3], np.full(len(c["ja"]), uc.OK, np.float32))
    assert uc.within(d, tol), (d, tol)
    trace = raw["landmark_cov"][:, :, [0, 2, 5]].sum(-1, dtype=np.float32)
    assert np.allclose(got["info"][:, 1], np.sqrt(trace.max(1)), rtol=2.0 ** -22, atol=0)


def test_the_free_finger_is_singular():
    """Every landmark of the index finger at weight 0: UT_COV_SINGULAR on every pose, +inf where promised, info[2] exactly 0 (a
    zero diagonal), and a finite pose_info and the pivot within the rule's bounds."""
    c, want = uc.case("free_finger"), uc.oracle("free_finger")
    raw = _raw(c)
    got = _unpacked(raw)
    d, d32 = uc.distance(c, got, want), uc.float32_distance("free_finger")
    tol = uc.bounds_from(d32)
    _show("free_finger", d, d32, tol)
    n = len(c["ja"])
    assert np.array_equal(got["info"][:, 3], np.full(n, uc.SINGULAR, np.float32)) and np.all(got["info"][:, 2] == 0)
    assert np.all(np.isposinf(got["info"][:, 1])) and np.all(np.isposinf(got["param_sigma"]))
    assert np.all(np.isposinf(raw["landmark_cov"][:, :, [0, 2, 5]])) and np.all(raw["landmark_cov"][:, :, [1, 3, 4]] == 0)
    assert np.all(np.isfinite(raw["pose_info"])) and np.array_equal(np.einsum("nii->ni", got["pose_info"]) == 0, uc.free_columns(c))
    assert d["pose_info"] <= tol["pose_info"] and d["pivot"] <= tol["pivot"] and d["rms"] <= tol["rms"]


# ----------------------------------------------------------------------------- 2. a pose is its own
@pytest.mark.parametrize("name", ["two_views", "mixed", "outliers_geman_mcclure"])
def test_a_pose_does_not_depend_on_its_batch(name):
    """n = 1, n = 5 (a partial workgroup behind a full one) and the 74: each pose of a batch has the bits of the same pose
    launched alone or in another batch; n_models 1 and n."""
    c = uc.case(name)
    whole = _raw(c)
    for sel in ([0], [17], list(range(5)), list(range(69, 74))):
        part = _raw(uc.subset(c, sel))
        assert _same_bits(part, uc.take(whole, sel)), (name, sel)


def test_unused_views_and_dead_windows_change_no_bit():
    """Padding trailing unused views, a -1 hole between the views, and NaN windows at weight 0: the bits of the plain case."""
    c = uc.subset(uc.case("two_views"), np.arange(9))
    plain = _raw(c)
    assert _same_bits(_raw(_padded(c, (0, 1))), plain) and _same_bits(_raw(_padded(c, (0, 2))), plain)
    assert _same_bits(_raw(_padded(c, (0, 1), 8)), plain)
    r = uc.subset(uc.case("ragged"), np.arange(9))
    off = (r["weights"] == 0) | (r["cam_rows"] < 0)[:, :, None]
    assert off.any() and np.isnan(r["window"][off]).any() and not np.isnan(r["window"][~off]).any()
    alive, dead = dict(r, window=r["window"].copy()), dict(r, window=r["window"].copy())
    alive["window"][off], dead["window"][off] = 0.0, np.nan
    assert _same_bits(_raw(dead), _raw(alive))


def test_pose_records_are_read_in_place():
    """Non-contiguous strides: the poses inside [n,60] records (angles at 3, the wrist's 16 floats at 30), and the strided
    outputs of a fit consumed in place, give the bits of the packed call."""
    c = uc.subset(uc.case("ragged"), np.arange(5))
    plain = _raw(c)
    rec = torch.full((5, 60), float("nan"), device=DEV)
    rec[:, 3:25], rec[:, 30:46] = _t(c["ja"]), _t(c["xf"]).reshape(5, 16)
    args, kw = _inputs(c)
    out = _native.pose_information_views(args[0], rec[:, 3:25], rec[:, 30:46], *args[3:], **kw, n=5, ja_stride=60, xf_stride=60)
    torch.cuda.synchronize()
    assert _same_bits(dict(zip(OUT, (o.cpu().numpy() for o in out))), plain)
    # the fit writes into the records, the information reads them there
    fit = pipeline.fit_keypoints_in_views(args[0], args[3], args[5], args[4], rec[:, 3:25].clone(), rec[:, 30:46].clone(), weights=kw["weights"],
                                          mirror=kw["mirror"], n=5, init_ja_stride=22, init_xf_stride=16, out=(rec[:, 3:25], rec[:, 30:46]),
                                          ja_stride=60, xf_stride=60, with_uncertainty=True)
    packed = _native.pose_information_views(args[0], rec[:, 3:25].contiguous(), rec[:, 30:46].contiguous(), *args[3:], **kw)
    torch.cuda.synchronize()
    want = hand.unpack_uncertainty(*packed)
    assert all(torch.equal(a, b) for a, b in zip(fit[-1], want)) and bool((fit[-1].status == uc.OK).all())


# ----------------------------------------------------------------------------- 3. refusals and errors
def test_a_negative_weight_refuses_the_pose():
    """A negative weight, a NaN window at a positive weight, fewer than 3 used landmarks and a bad angle_sigma (one whose 1 / sigma^2 overflows included) give
    UT_COV_REFUSED and zeros in every output of that pose; the other poses keep their bits."""
    c = uc.subset(uc.case("two_views"), np.arange(6))
    plain = _raw(c)
    bad = dict(c, weights=c["weights"].copy(), window=c["window"].copy())
    bad["weights"][1, 0, 3] = -1.0
    bad["window"][2, 1, np.nonzero(c["weights"][2, 1] > 0)[0][0]] = np.nan
    bad["weights"][4] = 0
    bad["weights"][4, 0, :2] = 1
    got = _raw(bad)
    for i in (1, 2, 4):
        assert got["info"][i, 3] == uc.REFUSED and not got["info"][i, :3].any()
        assert not any(got[k][i].any() for k in OUT[:4])
    assert _same_bits(uc.take(got, [0, 3, 5]), uc.take(plain, [0, 3, 5]))
    sigma = np.tile(uc.angle_sigma_from_limits(st.joint_limits()), (1, 1))
    for wrong in (0.0, -1.0, np.nan, np.inf, 1e-20):                                      # 1e-20: 1 / sigma^2 is not finite in fp32
        s = sigma.copy()
        s[0, 7] = wrong
        got = _raw(dict(c, angle_sigma=s))
        assert np.all(got["info"][:, 3] == uc.REFUSED) and not any(got[k].any() for k in OUT[:4])


def test_cam_rows_out_of_range_is_the_index_check():
    """An entry >= n_rows writes nothing for its pose - pre-filled outputs stay - and raises from the call with the checks
    synchronous, from poll_status with an engine in deferred-check mode; all outputs off is a ValueError before the call and
    UT_E_INVALID from the entry; n == 0 is UT_OK and writes nothing."""
    c = uc.subset(uc.case("two_views"), np.arange(5))
    rows = c["cam_rows"].copy()
    rows[2, 1] = len(c["table"])
    bad = dict(c, cam_rows=rows)
    plain = _raw(c)
    shapes = dict(pose_info=(5, 351), pivot=(5, 3), param_sigma=(5, 26), landmark_cov=(5, 21, 6), info=(5, 4))

    def buffers():
        return {k: torch.full(s, -7.0, device=DEV) for k, s in shapes.items()}

    def check(b):
        got = {k: v.cpu().numpy() for k, v in b.items()}
        assert all(np.all(got[k][2] == -7.0) for k in OUT)
        assert _same_bits(uc.take(got, [0, 1, 3, 4]), uc.take(plain, [0, 1, 3, 4]))

    args, kw = _inputs(bad)
    b = buffers()
    with pytest.raises(IndexError):
        _native.pose_information_views(*args, **kw, **b)
    torch.cuda.synchronize()
    check(b)
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            b = buffers()
            _native.pose_information_views(*args, **kw, **b, engine=eng)                  # no error here ...
            torch.cuda.synchronize()
            with pytest.raises(IndexError):
                eng.poll_status()                                                         # ... but here
            check(b)
    finally:
        eng.close()
    off = dict(pose_info=False, pivot=False, param_sigma=False, landmark_cov=False, info=False)
    with pytest.raises(ValueError):
        _native.pose_information_views(*_inputs(c)[0], **_inputs(c)[1], **off)
    lib = _native.load_library()
    a, k = _inputs(c)
    import ctypes

    def entry(n, *outs):
        return lib.ut_pose_information_views(None, a[0].data_ptr(), 1, a[3].data_ptr(), k["weights"].data_ptr(), a[4].data_ptr(), 2,
                                             a[5].data_ptr(), a[5].shape[0], 0, None, a[1].data_ptr(), 22, a[2].data_ptr(), 16,
                                             k["mirror"].data_ptr(), ctypes.c_float(1.0), 0, ctypes.c_float(3.0), n, *outs, None)

    assert entry(5, None, None, None, None, None) == -1 and "all five outputs" in lib.ut_last_error(None).decode()
    b = buffers()
    assert entry(0, *(b[name].data_ptr() for name in OUT)) == 0                           # n == 0: UT_OK, nothing launched
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in b.values())
    only = _native.pose_information_views(*_inputs(c)[0], **_inputs(c)[1], **dict(off, param_sigma=True))
    torch.cuda.synchronize()
    assert [o is None for o in only] == [True, True, False, True, True]
    assert np.array_equal(_bits(only[2].cpu().numpy()), _bits(plain["param_sigma"]))


def test_capturable_with_deferred_checks():
    """Captured under torch.cuda.graph with deferred checks on one set of windows and replayed on another: the eager bits."""
    first, c = uc.case("two_views"), uc.case("outliers_huber")
    args, kw = _inputs(c)
    kw = dict(kw, loss="huber", loss_scale=c["loss_scale"])
    win_first, win_then = _t(first["window"], torch.float64), _t(c["window"], torch.float64)
    win = win_first.clone()
    names = dict(pose_info=(74, 351), pivot=(74, 3), param_sigma=(74, 26), landmark_cov=(74, 21, 6), info=(74, 4))

    def buffers():
        return {k: torch.zeros(s, device=DEV) for k, s in names.items()}

    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            def launch(b):
                _native.pose_information_views(args[0], args[1], args[2], win, args[4], args[5], **kw, **b, engine=eng)

            eager, replayed = buffers(), buffers()
            launch(replayed)                              # every lazy initialisation happens before the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                launch(replayed)
            win.copy_(win_then)
            graph.replay()
            torch.cuda.synchronize()
            launch(eager)
            torch.cuda.synchronize()
            eng.poll_status()
    finally:
        eng.close()
    for k in eager:
        assert torch.equal(eager[k].view(torch.int32), replayed[k].view(torch.int32)), k
    assert _same_bits({k: v.cpu().numpy() for k, v in eager.items()}, _raw(c))


# ----------------------------------------------------------------------------- 4. the Python layers
def _frame_of(i):
    import triangulate_cases as tc
    z = np.load(tc.GOLDEN + "/projection_rec00.npz")
    return int(z["frame"][z["case_frame"]][i])


def test_hand_pose_uncertainty_views_is_the_native_entry():
    """hand.pose_uncertainty_views on CPU tensors with leading dims [2,37]: the native entry's outputs unpacked, the prior from
    hand.angle_sigma_from_limits; one-view hands are several times less certain in depth than across."""
    c = uc.case("free_finger_prior")
    raw = _unpacked(_raw(c))
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    model = model._replace(joint_limits=torch.from_numpy(np.concatenate([st.joint_limits(), np.zeros((2, 2), np.float32)])))
    sigma = hand.angle_sigma_from_limits(model)
    assert np.array_equal(sigma.numpy(), c["angle_sigma"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    lead = lambda a: t(a).reshape((2, 37) + a.shape[1:])
    unc = hand.pose_uncertainty_views(model, lead(c["ja"]), lead(c["xf"]), lead(c["window"]), lead(c["cam_rows"]), t(c["table"]),
                                      weights=lead(c["weights"]), angle_sigma=sigma, mirror=lead(c["mirror"]))
    assert unc.pose_info.shape == (2, 37, 26, 26) and unc.landmark_cov.shape == (2, 37, 21, 3, 3) and unc.status.shape == (2, 37)
    for got, k in ((unc.pose_info, "pose_info"), (unc.pivot, "pivot"), (unc.param_sigma, "param_sigma"), (unc.landmark_cov, "landmark_cov")):
        assert np.array_equal(_bits(got.numpy().reshape(raw[k].shape)), _bits(raw[k])), k
    assert bool((unc.status == hand.COV_OK).all())
    diag = unc.landmark_cov.diagonal(dim1=-2, dim2=-1)
    assert torch.allclose(unc.landmark_sigma, torch.sqrt(diag[..., 0] + diag[..., 1] + diag[..., 2]), rtol=2.0 ** -22, atol=0)      # the device's sqrt


def test_keywords_off_change_nothing_and_on_add_the_uncertainty():
    """pipeline.fit_keypoints_in_views(with_uncertainty=), tracker.refine_hand_pose_in_views(return_uncertainty=) and
    tracker.hand_pose_from_window_keypoints(return_uncertainty=): off, the bits and the length of the result without the keyword;
    on, the same pose and an uncertainty equal to a direct call at that pose with the same loss, weights and views."""
    c = rc.tracked_case("two", "geman_mcclure")
    fit_args = (_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["table"], torch.float64), _t(c["cam_rows"], torch.int32), _t(c["init"][0]),
                _t(c["init"][1]))
    kw = dict(weights=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64), loss="geman_mcclure", loss_scale=c["loss_scale"], with_inliers=True)
    base = pipeline.fit_keypoints_in_views(*fit_args, **kw)
    off = pipeline.fit_keypoints_in_views(*fit_args, **kw, with_uncertainty=False)
    on = pipeline.fit_keypoints_in_views(*fit_args, **kw, with_uncertainty=True)
    assert len(base) == len(off) == 4 and len(on) == 5
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), o.view(torch.int32)) for a, b, o in zip(base, off, on))
    direct = hand.unpack_uncertainty(*_native.pose_information_views(fit_args[0], on[0], on[1], fit_args[1], fit_args[3], fit_args[2],
                                                                     weights=kw["weights"], mirror=kw["mirror"], loss="geman_mcclure",
                                                                     loss_scale=c["loss_scale"]))
    assert isinstance(on[4], hand.PoseUncertainty) and all(torch.equal(a, b) for a, b in zip(on[4], direct))

    g, lab = vc.golden(), pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    for i in (3, 40):
        cams = [pipeline.cameras_for_frame(lab, _frame_of(i))[int(k)] for k in g["seeing"][i]]
        win, w, hand_idx = c["window"][i], c["weights"][i], int(g["hand"][i])
        init = tracker.SingleHandPose(joint_angles=c["init"][0][i], wrist_xform=c["init"][1][i], hand_confidence=1.0)
        plain = tracker.refine_hand_pose_in_views(model, cams, win, hand_idx, init, w, loss="geman_mcclure", loss_scale=rc.SCALE_PX)
        more = tracker.refine_hand_pose_in_views(model, cams, win, hand_idx, init, w, loss="geman_mcclure", loss_scale=rc.SCALE_PX,
                                                 return_uncertainty=True)
        assert len(plain) == 4 and len(more) == 5
        assert np.array_equal(_bits(plain[0].joint_angles), _bits(more[0].joint_angles)) and np.array_equal(_bits(plain[0].wrist_xform), _bits(more[0].wrist_xform))
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(plain[1:], more[1:4]))
        want = tracker.hand_pose_uncertainty_in_views(model, cams, win, hand_idx, more[0], w, "geman_mcclure", rc.SCALE_PX)
        assert all(np.array_equal(a, b) for a, b in zip(more[4], want)) and int(more[4].status) == hand.COV_OK
        assert more[4].pose_info.shape == (26, 26) and more[4].landmark_sigma.shape == (21,)
        two = tracker.hand_pose_from_window_keypoints(model, cams, win, hand_idx, w, init=init, refine_in_views=True, loss="geman_mcclure")
        three = tracker.hand_pose_from_window_keypoints(model, cams, win, hand_idx, w, init=init, refine_in_views=True, loss="geman_mcclure",
                                                        return_uncertainty=True)
        assert len(two) == 2 and len(three) == 3 and np.array_equal(_bits(two[0].joint_angles), _bits(three[0].joint_angles))
        assert np.array_equal(_bits(two[0].wrist_xform), _bits(three[0].wrist_xform)) and np.array_equal(two[1], three[1])
        want = tracker.hand_pose_uncertainty_in_views(model, cams, win, hand_idx, three[0], w, "geman_mcclure", 3.0)
        assert all(np.array_equal(a, b) for a, b in zip(three[2], want))
