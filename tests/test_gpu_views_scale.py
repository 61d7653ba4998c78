"""GPU tests of the pose fit in the views with the hand's scale as a parameter (csrc/fit_views_scale.hip through
ut_fit_pose_views_scale, hand.fit_landmarks_views_scale, hand.calibrate_scale_in_views, pipeline.calibrate_scale_in_views and
tracker.calibrate_hand_model_from_window_keypoints(refine_in_views=True)) against the float64 / float32 numpy restatement of
tests/views_scale_cases.py, which tests/test_views_scale_host.py checks.  The shapes are the 74 golden hands and slices of them.

Bounds (views_scale_cases.bounds_from): views_cases.bounds_from for angles, landmarks and px - the project's 1e-4 rad and 1e-3 mm
where the float32 restatement stays within a quarter of them, else 4 x the distance between the float32 and the float64
restatement on that case, the worse of the two float32 solvers of step_cases.SOLVERS - and the same rule for the scale and the
scale information with the floors 4e-6 / 1e-3 of tests/test_gpu_scale.py; computed here from the restatements, never from the
kernel's output, and printed.  Measured distances: DESIGN.md, "Hand scale from keypoints in the views"."""
import numpy as np
import pytest
import torch

import robust_cases as rc
import scale_cases as sc
import step_cases as st
import views_cases as vc
import views_scale_cases as vs
from absolutetrack_amd import _native, geometry, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("ja", "xf", "scale", "info", "residual", "inlier")


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(*(hm[k] for k in st.FIELDS))).reshape(-1, 321)


def _gpu(c, max_iters, pad_views=0):
    """The case on the GPU -> numpy dict(ja [n,22], xf [n,4,4], scale [n], info [n,6], residual [n,V,21], inlier [n,V,21]).
    pad_views: that many unused view slots (-1, NaN windows, NaN weights) behind the case's."""
    n, v = c["cam_rows"].shape
    win, rows, w = c["window"], c["cam_rows"], c["weights"]
    if pad_views:
        win = np.concatenate([win, np.full((n, pad_views, 21, 2), np.nan)], 1)
        rows = np.concatenate([rows, np.full((n, pad_views), -1, np.int32)], 1)
        w = np.concatenate([w, np.full((n, pad_views, 21), np.nan, np.float32)], 1)
    out = _native.fit_pose_views_scale(_blob(c["hm"]), _t(win, torch.float64), _t(rows, torch.int32), _t(c["table"], torch.float64),
                                       _t(c["init"][0]), _t(c["init"][1]), None if w is None else _t(w),
                                       None if c["limits"] is None else _t(c["limits"]),
                                       None if c["init_scale"] is None else _t(c["init_scale"]), c["mode"], _t(c["mirror"], torch.int64),
                                       c["t_scale"], max_iters, c["loss"], c["loss_scale"], residual=True, inlier=True)
    torch.cuda.synchronize()
    got = dict(zip(KEYS, (o.cpu().numpy() for o in out)))
    if pad_views:
        assert not got["residual"][:, v:].any() and not got["inlier"][:, v:].any()
        got["residual"], got["inlier"] = got["residual"][:, :v], got["inlier"][:, :v]
    return got


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _show(what, d, tol):
    print(f"{what}: angles {d['ang']:.2e} (bound {tol['ang']:.2e}) rad, landmarks {d['kp']:.2e} ({tol['kp']:.2e}) mm, rms / worst "
          f"{d['px']:.2e} ({tol['px']:.2e}) px, scale {d['scale']:.2e} ({tol['scale']:.2e}), information {d['scale_info']:.2e} "
          f"({tol['scale_info']:.2e}) relative")


def _views(c):
    return rc.views_of(c)


def _px_per_mm(c):
    """The largest norm of d window / d landmark over the case's used observations at its truth: px per mm."""
    jacs = _views(c).blocks(c["truth"], np.arange(len(c["truth"])))[6]
    return float(max(np.linalg.norm(j, axis=(-2, -1)).max() for j in jacs))


def _residual_of(c, res):
    """The float64 reprojection distances [n,V,21] of a result's pose on the model at the result's scale; 0 where unused or
    refused."""
    refused = (np.asarray(res["info"])[:, 3].astype(np.int64) & vs.REFUSED) != 0
    with np.errstate(all="ignore"):
        dist = _views(c).cost(vs.landmarks(c, res), np.arange(len(refused)), np.float64)[2]
    return np.where(refused[:, None, None], 0.0, dist)


# ----------------------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("k", vs.SCALES)
@pytest.mark.parametrize("name", vs.STEP_CASES)
def test_one_step(name, k):
    """max_iters = 1 from the +-0.2 rad / +-15 mm starts at scale 1 on exact windows of the model x k: pose, scale, rms, worst
    and the scale information against the float64 restatement's one step by the bound rule; one iteration, the restatement's
    status; angles 20 and 21 copied through; the residuals are those of the returned pose on the model at the returned scale -
    against the float64 forward function and projection of that state, within the project's 1e-3 mm for an fp32 forward function
    times the cameras' px per mm plus the rounding of the distance to fp32."""
    c = vs.case(name, k)
    n = len(c["mirror"])
    trace = []
    want = vs.restate(c, np.float64, 1, trace=trace)
    got = _gpu(c, 1)
    d, tol = vs.distance(c, got, want), vs.bounds_from(vs.float32_distance(c, want))
    _show(f"one step, {name} x {k} ({int(trace[0]['accept'].sum())} of {n} first trials accepted)", d, tol)
    assert np.array_equal(got["info"][:, 2], np.ones(n, np.float32)) and not got["info"][:, 5].any()
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32))
    assert np.array_equal(_bits(got["ja"][:, 20:]), _bits(c["init"][0][:, 20:]))
    assert np.array_equal(got["xf"][:, 3], np.tile(np.float32([0, 0, 0, 1]), (n, 1)))
    assert vs.within(d, tol), (d, tol)
    used = _views(c).used
    dist = _residual_of(c, got)
    off = float(np.abs(got["residual"] - dist).max())
    bound = st.KP_TOL_MM * _px_per_mm(c) + 2.0 ** -23 * float(dist.max())
    print(f"   residual against the returned state in float64: {off:.2e} px (bound {bound:.2e}), distances up to {dist.max():.1f} px")
    assert not got["residual"][~used].any() and off <= bound
    assert np.array_equal(got["inlier"], used.astype(np.float32))


# ----------------------------------------------------------------------------- 2. full fits
@pytest.mark.parametrize("k", vs.SCALES)
@pytest.mark.parametrize("name", ["two_views", "pinhole"])
def test_full_fits_recover_the_scale(name, k):
    """max_iters = 32 on exact two-view windows of the model x k, Fisheye62 and pinhole: every hand converges, none at a bound;
    per pose at most the float32 restatements' iterations plus the margin of views_cases.full_yardstick's rule (the largest
    distance of a float32 count from the float64 one, at least 2); scale and landmarks against the float64 restatement inside the
    bound rule's bounds; the scale information within INFO_RTOL of float64."""
    c = vs.case(name, k)
    runs = [vs.restate(c, dt, 32, how) for dt, how in st.RUNS]
    for r in runs:
        assert np.all(r["info"][:, 3] == vs.CONVERGED), name
    its32 = np.stack([r["info"][:, 2].astype(np.int64) for r in runs[:2]])
    it64 = runs[2]["info"][:, 2].astype(np.int64)
    margin = max(2, int(np.abs(its32 - it64).max()))
    got = _gpu(c, 32)
    its = got["info"][:, 2].astype(np.int64)
    d = vs.distance(c, got, runs[2])
    tol = vs.bounds_from(st.worst([vs.distance(c, r, runs[2]) for r in runs[:2]]))
    _show(f"full fits, {name} x {k}", d, tol)
    print(f"   scale error against {k}: GPU {np.abs(got['scale'].astype(np.float64) - k).max():.2e} (float32 restatements "
          f"{max(np.abs(r['scale'].astype(np.float64) - k).max() for r in runs[:2]):.2e}, float64 {np.abs(runs[2]['scale'] - k).max():.2e}); "
          f"iterations GPU mean {its.mean():.1f} max {its.max()}, float32 max {its32.max()}, float64 max {it64.max()}, margin {margin}, "
          f"largest GPU - float32 {int((its - its32.max(0)).max())}")
    assert np.array_equal(got["info"][:, 3], np.full(len(its), _native.UT_FITS_CONVERGED, np.float32))
    assert np.all(its <= its32.max(0) + margin)
    assert d["scale"] <= tol["scale"] and d["kp"] <= tol["kp"] and d["scale_info"] <= vs.INFO_RTOL


# ----------------------------------------------------------------------------- 3. fixed mode
@pytest.mark.parametrize("loss", ["squared", "huber"])
def test_fixed_mode_is_the_views_fit_on_the_scaled_model(loss):
    """Exact two-view windows of the model x 1.25, the scale fixed there: it comes back bit for bit, the information is 0, and
    pose, rms, worst, status, residual (and inlier with Huber at 3 px) are those of _native.fit_pose_views (fit_pose_views_robust)
    on the blob of scaled_hand_model(model, 1.25), by views_cases' bound rule on that case; the iteration counts lie within the
    margin of views_cases.full_yardstick's rule of each other.  Whether they are bit-identical is printed, not asserted: the
    source arithmetic is the same, the compiler's contraction need not be.  Measured, MI355X: not bit-identical (squared: angles
    4.3e-6 rad, landmarks 1.0e-4 mm, rms / worst 3.0e-5 px apart; on exact windows the count's tail is decided by rounding)."""
    base = vs.case("two_views", 1.25)
    n = len(base["mirror"])
    s = np.full(n, np.float32(1.25))
    c = dict(base, mode=vs.FIXED, init_scale=s, loss=loss)
    got = _gpu(c, 32)
    assert np.array_equal(_bits(got["scale"]), _bits(s)) and not got["info"][:, 4:].any()
    scaled = dict(base, hm=sc.scaled_model(base["hm"], s, np.float32), loss=loss)
    args = (_blob(scaled["hm"]), _t(c["window"], torch.float64), _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64),
            _t(c["init"][0]), _t(c["init"][1]), _t(c["weights"]))
    if loss == "squared":
        ref = _native.fit_pose_views(*args, mirror=_t(c["mirror"], torch.int64), residual=True)
        runs = [vc.restate(scaled, dt, 32, how) for dt, how in st.RUNS]
        tol = vc.bounds_from(st.worst([vc.distance(scaled, r, runs[2]) for r in runs[:2]]))
    else:
        ref = _native.fit_pose_views_robust(*args, mirror=_t(c["mirror"], torch.int64), loss=loss, loss_scale=c["loss_scale"], residual=True,
                                            inlier=True)
        runs = [rc.restate(scaled, dt, 32, how) for dt, how in st.RUNS]
        tol = rc.bounds_from(st.worst([rc.distance(scaled, r, runs[2]) for r in runs[:2]]))
    its = [r["info"][:, 2] for r in runs]
    margin = max(2, int(max(np.abs(its[0] - its[2]).max(), np.abs(its[1] - its[2]).max())))      # views_cases.full_yardstick's rule
    torch.cuda.synchronize()
    ref = dict(zip(("ja", "xf", "info", "residual", "inlier"), (o.cpu().numpy() for o in ref)))
    mine = dict(got, info=got["info"][:, :4])
    d = vc.distance(scaled, mine, ref)
    same = all(np.array_equal(_bits(mine[k]), _bits(ref[k])) for k in ref)
    print(f"fixed at 1.25, {loss}: against the views fit on the scaled blob angles {d['ang']:.2e} (bound {tol['ang']:.2e}) rad, landmarks "
          f"{d['kp']:.2e} ({tol['kp']:.2e}) mm, rms / worst {d['px']:.2e} ({tol['px']:.2e}) px; bit-identical: {same}")
    first = dict(_gpu(c, 1), info=None)
    ref1 = (_native.fit_pose_views if loss == "squared" else _native.fit_pose_views_robust)(*args, mirror=_t(c["mirror"], torch.int64), max_iters=1,
                                                                                           **({} if loss == "squared" else dict(loss=loss)))
    print(f"   after one step the pose is bit-identical: {all(np.array_equal(_bits(first[k]), _bits(ref1[i].cpu().numpy())) for i, k in enumerate(('ja', 'xf')))}; "
          f"iterations differ by at most {int(np.abs(mine['info'][:, 2] - ref['info'][:, 2]).max())} (margin {margin})")
    assert np.array_equal(mine["info"][:, 3], ref["info"][:, 3]) and np.all(np.abs(mine["info"][:, 2] - ref["info"][:, 2]) <= margin)
    assert vc.within(d, tol)
    assert np.abs(mine["residual"] - ref["residual"]).max() <= tol["px"] + tol["kp"] * _px_per_mm(scaled)
    if loss != "squared":
        assert np.abs(mine["inlier"] - ref["inlier"]).max() <= tol["inlier"]


# ----------------------------------------------------------------------------- 4. one view
def test_one_view_says_nothing_about_the_scale():
    """The best view alone, exact windows of the model x 1.25.  Free, max_iters = 32: the rms against the float64 restatement's
    inside the px bound, and every hand's information (0 allowed) below 1e-3 of the same hand's two-view information from the
    same kernel.  The same hands fixed at the true scale, one step from the cases' starts: the float64 restatement by the bound
    rule."""
    one, two = vs.case("best_view", 1.25), vs.case("two_views", 1.25)
    want = vs.restate(one, np.float64, 32)
    # the float32 restatement with numpy's LU alone: the scale is a direction one view leaves flat, the float32 matrix is not
    # positive definite to numpy's Cholesky, which raises where the kernel takes a bad pivot as a failed solve and goes on
    tol = vs.bounds_from(vs.distance(one, vs.restate(one, np.float32, 32, "lu"), want))
    got, got2 = _gpu(one, 32), _gpu(two, 32)
    off = float(np.abs(got["info"][:, 0] - want["info"][:, 0]).max())
    ratio = got["info"][:, 4].astype(np.float64) / got2["info"][:, 4]
    print(f"one view, free: rms up to {got['info'][:, 0].max():.1e} px ({off:.1e} from float64, bound {tol['px']:.1e}), scale off by up to "
          f"{np.abs(got['scale'] - 1.25).max():.3f}, information {got['info'][:, 4].min():.3g} .. {got['info'][:, 4].max():.3g} against "
          f"{got2['info'][:, 4].min():.3g} .. {got2['info'][:, 4].max():.3g} in two views: ratio at most {ratio.max():.1e}")
    assert off <= tol["px"] and np.all(got2["info"][:, 4] > 0) and np.all(got["info"][:, 4] >= 0) and np.all(ratio < 1e-3)
    fixed = dict(one, mode=vs.FIXED, init_scale=np.full(len(one["mirror"]), np.float32(1.25)))
    want = vs.restate(fixed, np.float64, 1)
    got = _gpu(fixed, 1)
    d, tol = vs.distance(fixed, got, want), vs.bounds_from(vs.float32_distance(fixed, want))
    _show("one view, fixed at the true scale, one step", d, tol)
    assert np.array_equal(got["info"][:, 2:4], want["info"][:, 2:4].astype(np.float32)) and vs.within(d, tol)


# ----------------------------------------------------------------------------- 5. decisions
def _decision_case():
    """tests/test_gpu_views.py's decision case on poses 0 - 7, and start scales that are refused on poses 8 - 10."""
    c = vs.subset(vs.case("two_views", 0.8), np.arange(12))
    win, w, rows, s = c["window"].copy(), c["weights"].copy(), c["cam_rows"].copy(), c["init_scale"].copy()
    w[0, 1, 4] = 0
    win[0, 1, 4] = np.nan                         # a NaN window at weight 0
    w[1, 0, 3] = -1.0                             # a negative weight
    w[2, 1, 7] = np.nan                           # a NaN weight
    win[3, 0, 5, 1] = np.inf                      # a non-finite window at a positive weight
    w[4] = 0
    w[4, 0, [2, 9]] = 1                           # two landmarks with a used observation
    rows[5, 1] = -1
    w[5, 1] = np.nan                              # the weights of an unused view are not read
    s[8], s[9], s[10] = np.nan, 0.1, 5.0          # not finite, below UT_SCALE_MIN, above UT_SCALE_MAX
    return dict(c, window=win, weights=w, cam_rows=rows, init_scale=s)


def test_refusals_keep_the_start_at_scale_1():
    c = _decision_case()
    got, want = _gpu(c, 32), vs.restate(c, np.float64, 32)
    refused = [1, 2, 3, 4, 8, 9, 10]
    assert np.array_equal(got["info"][:, 3].astype(int), [1, 4, 4, 4, 4, 1, 1, 1, 4, 4, 4, 1])
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3].astype(np.float32))
    for k in KEYS:
        assert np.isfinite(got[k]).all(), k
    assert np.array_equal(_bits(got["ja"][refused]), _bits(c["init"][0][refused]))
    assert np.array_equal(_bits(got["xf"][refused]), _bits(c["init"][1][refused]))
    assert np.array_equal(got["scale"][refused], np.ones(7, np.float32))
    assert not got["info"][refused][:, [0, 1, 2, 4, 5]].any() and not got["residual"][refused].any() and not got["inlier"][refused].any()
    assert not got["residual"][5, 1].any()
    err = np.linalg.norm(vs.landmarks(c, got) - c["truth"], axis=-1).max(1)
    two = [0, 6, 7, 11]                           # pose 5 is left with one view: it converges, to a scale that means nothing
    assert err[two].max() <= st.KP_TOL_MM and np.abs(got["scale"][two] - 0.8).max() <= vs.SCALE_TOL
    assert got["info"][5, 4] < 1e-3 * got["info"][two, 4].min()
    garbage = c["window"].copy()
    garbage[0, 1, 4] = 123.5
    assert _same_bits(got, _gpu(dict(c, window=garbage), 32))
    group, _ = _native.pool_scale(_t(got["scale"]), _t(got["info"]), 12)
    assert int(group[0, 3]) == 5 and abs(np.log(float(group[0, 0]) / 0.8)) < 1e-4


def test_a_fit_driven_to_the_bound_is_flagged_and_not_pooled():
    """Exact windows of the model x 4.4 from a start scale of 3.9: the scale ends at UT_SCALE_MAX with UT_FITS_AT_BOUND, as in the
    float64 restatement, and ut_pool_scale uses none of these poses."""
    c = vs.subset(vs.case("two_views", 4.4), np.arange(6))
    c["init_scale"] = np.full(6, np.float32(3.9))
    got, want = _gpu(c, 32), vs.restate(c, np.float64, 32)
    print(f"driven to the bound: scale {got['scale']}, status {got['info'][:, 3].astype(int)} (float64 {want['info'][:, 3].astype(int)})")
    assert np.all(want["scale"] == 4.0) and np.all(want["info"][:, 3].astype(int) & vs.AT_BOUND)
    assert np.array_equal(got["scale"], np.full(6, np.float32(_native.UT_SCALE_MAX)))
    assert np.all(got["info"][:, 3].astype(int) & _native.UT_FITS_AT_BOUND) and np.isfinite(got["info"]).all()
    group, pose_scale = _native.pool_scale(_t(got["scale"]), _t(got["info"]), 6)
    assert group.cpu().tolist() == [[1.0, float("inf"), 0.0, 0.0]] and bool((pose_scale == 1).all())


def test_cam_rows_out_of_range_is_the_index_check():
    """A cam_rows entry outside [-1, n_rows): nothing is written for that pose, `scale` included, and the call raises IndexError
    with synchronous checks; with an engine that runs deferred checks the call returns and poll_status raises."""
    c = vs.subset(vs.case("two_views", 0.8), np.arange(5))
    rows = c["cam_rows"].copy()
    rows[2, 1] = len(c["table"])
    args = (_blob(c["hm"]), _t(c["window"], torch.float64), _t(rows, torch.int32), _t(c["table"], torch.float64), _t(c["init"][0]),
            _t(c["init"][1]), _t(c["weights"]))

    def buffers():
        return dict(out=(torch.full((5, 22), 7.0, device=DEV), torch.full((5, 4, 4), 7.0, device=DEV)), scale=torch.full((5,), 7.0, device=DEV),
                    info=torch.full((5, 6), 7.0, device=DEV), residual=torch.full((5, 2, 21), 7.0, device=DEV),
                    inlier=torch.full((5, 2, 21), 7.0, device=DEV))

    def untouched(b):
        for t in b["out"] + (b["scale"], b["info"], b["residual"], b["inlier"]):
            assert bool((t[2] == 7.0).all()) and bool((t[[0, 1, 3, 4]] != 7.0).any())

    b = buffers()
    with pytest.raises(IndexError):
        _native.fit_pose_views_scale(*args, mirror=_t(c["mirror"], torch.int64), **b)
    torch.cuda.synchronize()
    untouched(b)
    ok = _gpu(c, 32)
    assert np.array_equal(_bits(b["out"][0].cpu().numpy()[[0, 1, 3, 4]]), _bits(ok["ja"][[0, 1, 3, 4]]))
    assert np.array_equal(_bits(b["scale"].cpu().numpy()[[0, 1, 3, 4]]), _bits(ok["scale"][[0, 1, 3, 4]]))
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            b = buffers()
            _native.fit_pose_views_scale(*args, mirror=_t(c["mirror"], torch.int64), engine=eng, **b)      # no error here ...
            torch.cuda.synchronize()
            with pytest.raises(IndexError):
                eng.poll_status()                                                                           # ... but here
    finally:
        eng.close()
    untouched(b)
    with pytest.raises(ValueError):
        _native.fit_pose_views_scale(args[0], args[1], _t(c["cam_rows"], torch.int32), args[3], None, None)


# ----------------------------------------------------------------------------- 6. batch independence
@pytest.mark.parametrize("name,loss", [("two_views", "squared"), ("ragged", "huber")])
def test_padding_and_batches_leave_the_bits(name, loss):
    """Two unused view slots behind the case's (-1 rows, NaN windows, NaN weights) and the batch of 74 split as 1 + 73 and as
    3 + 71 - across the workgroups of three poses - leave the bits of every output unchanged."""
    c = dict(vs.case(name, 1.25), loss=loss)
    whole = _gpu(c, 32)
    assert _same_bits(whole, _gpu(c, 32, pad_views=2))
    for cut in (1, 3):
        parts = [_gpu(vs.subset(c, np.arange(0, cut)), 32), _gpu(vs.subset(c, np.arange(cut, 74)), 32)]
        assert _same_bits({k: np.concatenate([p[k] for p in parts]) for k in KEYS}, whole), cut


# ----------------------------------------------------------------------------- 7. the chain in a graph
def test_the_chain_is_capturable_with_deferred_checks():
    """Free pass -> ut_pool_scale -> fixed pass, captured in one graph with deferred checks on windows of the model x 0.8 and
    replayed on windows of the model x 1.1: the bits of the eager chain on those, and the pooled scale of the 74 exact two-view
    hands within SCALE_TOL of 1.1."""
    first, c = vs.case("two_views", 0.8), vs.case("two_views", 1.1)
    blob, rows, table = _blob(c["hm"]), _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64)
    ja0, xf0, w, mirror = _t(c["init"][0]), _t(c["init"][1]), _t(c["weights"]), _t(c["mirror"], torch.int64)
    win_first, win_then = _t(first["window"], torch.float64), _t(c["window"], torch.float64)
    win = win_first.clone()

    def buffers():
        z = lambda *shape: torch.zeros(*shape, device=DEV)
        return dict(ja=z(74, 22), xf=z(74, 4, 4), s=z(74), info=z(74, 6), group=z(1, 4), ps=z(74), ja2=z(74, 22), xf2=z(74, 4, 4), s2=z(74),
                    info2=z(74, 6))

    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            def chain(b):
                _native.fit_pose_views_scale(blob, win, rows, table, ja0, xf0, w, mirror=mirror, out=(b["ja"], b["xf"]), scale=b["s"],
                                             info=b["info"], engine=eng)
                _native.pool_scale(b["s"], b["info"], 74, group=b["group"], pose_scale=b["ps"])
                _native.fit_pose_views_scale(blob, win, rows, table, b["ja"], b["xf"], w, init_scale=b["ps"], scale_mode=_native.UT_SCALE_FIXED,
                                             mirror=mirror, out=(b["ja2"], b["xf2"]), scale=b["s2"], info=b["info2"], engine=eng)

            eager, replayed = buffers(), buffers()
            chain(replayed)                               # every lazy initialisation happens before the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                chain(replayed)
            win.copy_(win_then)
            graph.replay()
            torch.cuda.synchronize()
            chain(eager)
            torch.cuda.synchronize()
            eng.poll_status()
    finally:
        eng.close()
    for name in eager:
        assert torch.equal(eager[name].view(torch.int32), replayed[name].view(torch.int32)), name
    pooled = float(eager["group"][0, 0])
    print(f"captured chain: pooled scale {pooled:.7f} (1.1: {pooled - 1.1:+.2e}), {int(eager['group'][0, 3])} poses used, fixed pass rms up "
          f"to {float(eager['info2'][:, 0].max()):.1e} px")
    assert abs(pooled - 1.1) <= vs.SCALE_TOL and int(eager["group"][0, 3]) == 74
    assert torch.equal(eager["s2"], eager["ps"]) and bool((eager["ps"] == eager["group"][0, 0]).all())


# ----------------------------------------------------------------------------- 8. noisy detections
def _calibration_distance(c, got, want):
    """A calibration against another: the fixed pass by views_scale_cases.distance, and |pooled scale|, sigma and scatter
    (relative) and the number of poses used of the pool."""
    d = vs.distance(c, got["fixed"], want["fixed"])
    a, b = np.asarray(got["stats"], np.float64), np.asarray(want["stats"], np.float64)
    return dict(ang=d["ang"], kp=d["kp"], px=d["px"], pooled=abs(a[0] - b[0]), sigma=abs(a[1] - b[1]) / b[1], scatter=abs(a[2] - b[2]) / b[2],
                used=abs(a[3] - b[3]))


def _calibration_bounds(d32):
    """The bound rule on a calibration: views_cases.bounds_from for the fixed pass; st.FLOAT32_FACTOR x the float32 restatements'
    distance for the pool's figures, with the floors SCALE_TOL (pooled scale) and INFO_RTOL (sigma and scatter, relative)."""
    f = st.FLOAT32_FACTOR
    return dict(vc.bounds_from(d32), pooled=max(vs.SCALE_TOL, f * d32["pooled"]), sigma=max(vs.INFO_RTOL, f * d32["sigma"]),
                scatter=max(vs.INFO_RTOL, f * d32["scatter"]), used=f * d32["used"])


def _calibrate_gpu(c, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    cal = hand.calibrate_scale_in_views(model, t(c["window"]), t(c["cam_rows"]), t(c["table"]), (t(c["init"][0]), t(c["init"][1])),
                                        t(c["init_scale"]), weights=t(c["weights"]), mirror=t(c["mirror"]), **kw)
    fixed = dict(ja=cal.joint_angles.numpy(), xf=cal.wrist_transforms.numpy(), scale=cal.pose_scale.numpy(), info=cal.info.numpy())
    return cal, dict(stats=cal.stats.numpy(), fixed=fixed)


def test_noisy_calibration_in_the_views():
    """1 px noise (seed 0) on the two seeing views of the 74 golden hands, the model at 1.1, starts from the float64 3-D chain:
    hand.calibrate_scale_in_views - pooled scale, sigma, scatter, poses used and the poses refitted at the pooled scale - against
    the float64 restatement's chain by the bound rule; pipeline.calibrate_scale_in_views gives its bits."""
    c = vs.noisy_case(1.0, 0)
    want = vs.calibrate(c, np.float64)
    d32 = st.worst([_calibration_distance(c, vs.calibrate(c, np.float32, solver=s), want) for s in st.SOLVERS])
    cal, got = _calibrate_gpu(c)
    d, tol = _calibration_distance(c, got, want), _calibration_bounds(d32)
    chain = sc.pool(c["chain"]["scale"], c["chain"]["info"], 74)[0]
    print(f"noisy calibration: pooled scale {got['stats'][0]:.6f} (float64 {want['stats'][0]:.6f}, the 3-D chain it starts from {chain[0]:.6f}, "
          f"truth 1.1), used {got['stats'][3]:.0f} (float64 {want['stats'][3]:.0f}, chain {chain[3]:.0f})")
    print("   " + ", ".join(f"{k} {d[k]:.2e} (bound {tol[k]:.2e})" for k in d))
    assert all(d[k] <= tol[k] for k in d), (d, tol)
    assert cal.hand_model is not None and float(cal.scale) == got["stats"][0] and bool((cal.pose_scale == cal.scale).all())
    out = pipeline.calibrate_scale_in_views(_blob(c["hm"]), _t(c["window"], torch.float64), _t(c["table"], torch.float64),
                                            _t(c["cam_rows"], torch.int32), _t(c["init"][0]), _t(c["init"][1]), _t(c["init_scale"]),
                                            weights=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64))
    mine = dict(zip(("stats", "ja", "xf", "scale", "info"), (o.cpu().numpy() for o in out)))
    assert np.array_equal(_bits(mine["stats"][0]), _bits(got["stats"])) and _same_bits(mine, got["fixed"], ("ja", "xf", "scale", "info"))
    with pytest.raises(ValueError, match="no usable pose"):
        _calibrate_gpu(dict(c, weights=np.zeros_like(c["weights"])))


HUBER_FACTOR = 14.3


def test_huber_calibration_survives_displaced_detections():
    """The same noisy hands with six detections per hand (three per view) moved 40 px, Huber at 3 px in both passes: the pooled
    scale stays within HUBER_FACTOR x st.FLOAT32_FACTOR x the clean run's distance from 1.1.  HUBER_FACTOR is the float64 robust
    restatement's: its pooled scale lies 2.41e-2 from 1.1 on these detections (9 poses usable: Huber keeps pulling at the
    outliers along the valley in depth and most fits run to max_iters) against 1.69e-3 on the clean ones (70 usable), 14.2 x; the
    float32 restatements 3.2e-2 and 3.1e-2 (23 and 22 usable).  The squared loss on the same detections is printed for contrast:
    float64 3.2e-1.  Measured, MI355X: 3.42e-2 with 22 poses used, bound 9.78e-2; squared 2.65e-1."""
    clean, dirty = vs.noisy_case(1.0, 0), vs.noisy_case(1.0, 0, 6)
    assert int(dirty["displaced"].sum()) == 6 * 74
    d_clean = abs(float(_calibrate_gpu(clean)[1]["stats"][0]) - vs.NOISY_SCALE)
    huber = _calibrate_gpu(dict(dirty, loss="huber"), loss="huber", loss_scale=rc.SCALE_PX)[1]["stats"]
    squared = _calibrate_gpu(dirty)[1]["stats"]
    d_huber = abs(float(huber[0]) - vs.NOISY_SCALE)
    bound = HUBER_FACTOR * st.FLOAT32_FACTOR * d_clean
    print(f"six detections per hand moved 40 px: pooled scale off 1.1 by {d_huber:.2e} with Huber at 3 px ({huber[3]:.0f} poses used; bound "
          f"{bound:.2e} = {HUBER_FACTOR} x {st.FLOAT32_FACTOR} x the clean run's {d_clean:.2e}), by {abs(float(squared[0]) - 1.1):.2e} with the "
          f"squared loss ({squared[3]:.0f} used)")
    assert d_huber <= bound


def test_tracker_calibration_refined_in_the_views():
    """20 left-hand label poses carried rigidly into the camera rig of frame 0, through ut_fk on the model x 1.1 and
    ut_project_points into the four cameras, plus 1 px noise (seed 0).  refine_in_views=False is the default call and the old
    path - triangulation, then hand.calibrate_scale - bit for bit.  refine_in_views=True is hand.calibrate_scale_in_views started
    from that path's free pass, bit for bit, and meets the float64 restatement's chain from the same start by the bound rule."""
    import mesh_cases as mc
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand_idx = mc.label_poses(lab)
    sel = (2 * np.arange(0, 369, 6))[np.arange(0, 60, 3)]
    assert np.all(hand_idx[sel] == 0) and len(sel) == 20
    rigs = lab["camera_to_world_transforms"].astype(np.float64)
    xf0 = rigs[0, 0] @ np.linalg.inv(rigs[sel // 2, 0]) @ xf[sel].astype(np.float64)
    cams = pipeline.cameras_for_frame(lab, 0)
    table = np.stack([geometry.pack_camera_model(cam) for cam in cams])
    blob11 = _blob(sc.scaled_model(hm, np.full(1, np.float32(1.1)), np.float32))
    lm = _native.fk_stateless(blob11, _t(ja[sel]), _t(xf0))
    rows = torch.arange(4, dtype=torch.int32, device=DEV)[None].expand(20, -1).contiguous()
    win, _, flags = _native.project_points(lm, rows, _t(table, torch.float64), int(cams[0].width), int(cams[0].height))
    weights = (flags == 3).float().cpu().numpy()
    win = np.where(weights[..., None] > 0, win.cpu().numpy(), 0.0) + np.random.default_rng(0).normal(0.0, 1.0, (20, 4, 21, 2))
    assert np.all(weights.sum(1) >= 2)
    # the default, and the old path written out
    plain = tracker.calibrate_hand_model_from_window_keypoints(model, cams, win, 0, weights=weights)
    off = tracker.calibrate_hand_model_from_window_keypoints(model, cams, win, 0, weights=weights, refine_in_views=False)
    pts, info, _ = _native.triangulate_points(_t(win, torch.float64), rows, _t(table, torch.float64), weights=_t(weights))
    sigma = info[..., 1].double()
    ok = torch.isfinite(sigma) & (sigma > 0)
    best = torch.where(ok, sigma, torch.full_like(sigma, float("inf"))).amin(1, keepdim=True)
    lw = torch.where(ok, (best / torch.where(ok, sigma, torch.ones_like(sigma))) ** 2, torch.zeros_like(sigma)).float()
    mirror = torch.zeros(20, dtype=torch.int64, device=DEV)
    old = hand.calibrate_scale(model, pts.float(), lw, mirror)
    fields = ("scale", "stats", "joint_angles", "wrist_transforms", "info", "pose_scale")
    for other in (off, old):
        for f in fields:
            assert torch.equal(getattr(plain, f).view(torch.int32), getattr(other, f).cpu().view(torch.int32)), f
    # refined in the views
    fine = tracker.calibrate_hand_model_from_window_keypoints(model, cams, win, 0, weights=weights, refine_in_views=True)
    start = hand.calibrate_scale(model, pts.float(), lw, mirror, refit=False)
    direct = hand.calibrate_scale_in_views(model, _t(win, torch.float64), rows, _t(table, torch.float64),
                                           (start.joint_angles, start.wrist_transforms), start.pose_scale, weights=_t(weights), mirror=mirror)
    for f in fields:
        assert torch.equal(getattr(fine, f).view(torch.int32), getattr(direct, f).cpu().view(torch.int32)), f
    c = dict(hm=hm, window=win, cam_rows=rows.cpu().numpy(), table=table, weights=weights, mirror=np.zeros(20, np.int64), t_scale=1.0,
             limits=None, init=(start.joint_angles.cpu().numpy(), start.wrist_transforms.cpu().numpy()),
             init_scale=start.pose_scale.cpu().numpy(), mode=vs.FREE, loss="squared", loss_scale=rc.SCALE_PX)
    want = vs.calibrate(c, np.float64)
    d32 = st.worst([_calibration_distance(c, vs.calibrate(c, np.float32, solver=s), want) for s in st.SOLVERS])
    got = dict(stats=fine.stats.numpy(), fixed=dict(ja=fine.joint_angles.numpy(), xf=fine.wrist_transforms.numpy(),
                                                    scale=fine.pose_scale.numpy(), info=fine.info.numpy()))
    d, tol = _calibration_distance(c, got, want), _calibration_bounds(d32)
    print(f"tracker, 20 frames in four cameras, 1 px noise: scale {float(plain.scale):.5f} from the 3-D chain ({int(plain.stats[3])} poses "
          f"used), {float(fine.scale):.5f} refined in the views ({int(fine.stats[3])} used; float64 {want['stats'][0]:.5f}), truth 1.1")
    print("   " + ", ".join(f"{k} {d[k]:.2e} (bound {tol[k]:.2e})" for k in d))
    assert all(d[k] <= tol[k] for k in d), (d, tol)
    assert torch.equal(fine.hand_model.joint_rest_positions, model.joint_rest_positions * float(fine.scale))
