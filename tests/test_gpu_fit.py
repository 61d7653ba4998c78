"""GPU tests of the pose fit (csrc/fit.hip through ut_fit_pose, hand.fit_landmarks and the tracker functions) against the
float64 forward function and the float64 / float32 numpy solvers of tests/fit_cases.py, which tests/test_fit_host.py checks.

Bounds: 1e-3 mm on landmarks and 1e-4 rad on angles, the project's keypoint and angle tolerances.  Targets are the float64
forward function of the label poses, handed to the kernel as float32 (that cast alone moves a coordinate by up to 1.5e-5 mm
at 300 mm)."""
import os

import numpy as np
import pytest
import torch

import fit_cases as fc
import mesh_cases as mc
from absolutetrack_amd import _native, hand, pipeline, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KP_TOL_MM, ANGLE_TOL_RAD = 1e-3, 1e-4


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"], hm["landmark_rest_positions"],
                                      hm["landmark_rest_bone_weights"], hm["landmark_rest_bone_indices"])).reshape(-1, 321)


def _fit(blob, targets, mirror, weights=None, limits=None, init=None, **kw):
    """ut_fit_pose on numpy inputs -> numpy (joint_angles [n,22], wrist [n,4,4], info [n,4])."""
    ja, xf, info = _native.fit_pose(blob, _t(targets), None if weights is None else _t(weights),
                                    None if limits is None else _t(limits), None if init is None else _t(init[0]),
                                    None if init is None else _t(init[1]), _t(mirror, torch.int64), **kw)
    torch.cuda.synchronize()
    return ja.cpu().numpy(), xf.cpu().numpy(), info.cpu().numpy()


def _fk64(hm, ja, xf, mirror, t_scale=1.0):
    return fc.forward(hm, ja.astype(np.float64), fc.effective_wrist(xf.astype(np.float64), mirror, t_scale, np.float64))


def _fk_gpu(blob, ja, xf, mirror, t_scale=1.0):
    return _native.fk_stateless(blob, _t(ja), _t(xf), mirror=_t(mirror, torch.int64), t_scale=t_scale).cpu().numpy()


def _dist(a, b):
    return np.linalg.norm(a.astype(np.float64) - b, axis=-1)


@pytest.fixture(scope="module")
def rec00():
    """All 369 x 2 label poses of the recording (right hands through the mirror flag), their float64 landmarks, and the
    cold-start fit of those on the GPU, shared by the tests that look at it."""
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand_idx = mc.label_poses(lab)
    targets = fc.forward(hm, ja, fc.effective_wrist(xf, hand_idx, 1.0, np.float64))
    blob = _blob(hm)
    got = _fit(blob, targets, hand_idx)
    return dict(hm=hm, blob=blob, ja=ja, xf=xf, hand=hand_idx, targets=targets, got=got, limits=hm["joint_limits"][:20])


def _check_recovered(r, sel, ja, xf, what):
    """The bounds of the exact-target tests on poses `sel`: float64 FK of the result and ut_fk of the result within 1e-3 mm
    of the targets on every landmark, angles within 1e-4 rad of the labels modulo 2 pi."""
    kp = _dist(_fk64(r["hm"], ja, xf, r["hand"][sel]), r["targets"][sel]).max()
    kp_gpu = _dist(_fk_gpu(r["blob"], ja, xf, r["hand"][sel]), r["targets"][sel]).max()
    ang = fc.angle_distance(ja[:, :20], r["ja"][sel, :20]).max()
    print(f"{what}: float64 FK of the fit {kp:.3e} mm, ut_fk of the fit {kp_gpu:.3e} mm, angles {ang:.3e} rad")
    assert kp <= KP_TOL_MM and kp_gpu <= KP_TOL_MM and ang <= ANGLE_TOL_RAD
    return kp, ang


def test_exact_targets_cold_start(rec00):
    r = rec00
    ja, xf, info = r["got"]
    every = np.arange(738)
    print(f"iterations: max {int(info[:, 2].max())}, mean {info[:, 2].mean():.2f}; status counts {np.bincount(info[:, 3].astype(int))}")
    assert np.all(info[:, 3] == _native.UT_FIT_CONVERGED)
    _check_recovered(r, every, ja, xf, "738 label poses, cold start, GPU")
    ja32, xf32, info32 = fc.fit(r["hm"], r["targets"], mirror=r["hand"], dtype=np.float32)
    print(f"float32 numpy yardstick: {_dist(_fk64(r['hm'], ja32, xf32, r['hand']), r['targets']).max():.3e} mm, "
          f"{fc.angle_distance(ja32[:, :20], r['ja'][:, :20]).max():.3e} rad, max {int(info32[:, 2].max())} iterations")
    assert np.abs(ja[:, :20]).max() <= np.pi and np.array_equal(ja[:, 20:], np.zeros((738, 2), np.float32))
    assert np.array_equal(xf[:, 3], np.tile(np.float32([0, 0, 0, 1]), (738, 1)))
    # info is what the kernel saw: rms <= worst <= the bound
    assert np.all(info[:, 0] <= info[:, 1]) and info[:, 1].max() <= KP_TOL_MM


def test_stored_keypoints_of_the_reference(golden_dir):
    """The reference's stored gt_keypoints of three recordings, each with its own skeleton, valid frames only: fit -> ut_fk
    comes back within 1e-3 mm."""
    g = np.load(os.path.join(golden_dir, "fk_user05.npz"))
    n_checked = 0
    for rec in ("00", "02", "11"):
        p = f"r{rec}."
        hm = mc.skeleton(g, p + "hm.")
        valid = g[p + "valid_tracking"]
        hand_idx, frame = np.nonzero(valid)
        kp = g[p + "gt_keypoints"][hand_idx, frame]
        ja, xf, info = _fit(_blob(hm), kp, hand_idx)
        err = _dist(_fk_gpu(_blob(hm), ja, xf, hand_idx), kp).max()
        print(f"recording {rec}: {len(kp)} valid hand-frames, fit -> ut_fk vs stored keypoints {err:.3e} mm, "
              f"max {int(info[:, 2].max())} iterations, status counts {np.bincount(info[:, 3].astype(int))}")
        assert err <= KP_TOL_MM
        n_checked += len(kp)
    assert n_checked > 250


def test_warm_start_from_perturbed_labels(rec00):
    r = rec00
    rng = np.random.default_rng(20)
    ja0 = r["ja"].copy()
    ja0[:, :20] += rng.uniform(-0.4, 0.4, (738, 20))
    xf0 = r["xf"].copy()
    xf0[:, :3, :3] = fc._rodrigues(rng.uniform(-0.3, 0.3, (738, 3))) @ xf0[:, :3, :3]
    xf0[:, :3, 3] += rng.uniform(-30, 30, (738, 3))
    ja, xf, info = _fit(r["blob"], r["targets"], r["hand"], init=(ja0, xf0), max_iters=16)
    print(f"warm start: iterations max {int(info[:, 2].max())}, mean {info[:, 2].mean():.2f}; status counts "
          f"{np.bincount(info[:, 3].astype(int))}")
    assert info[:, 2].max() <= 16 and np.all(info[:, 3] == _native.UT_FIT_CONVERGED)
    _check_recovered(r, np.arange(738), ja, xf, "738 label poses, perturbed warm start, GPU")
    assert np.array_equal(ja[:, 20:], ja0[:, 20:].astype(np.float32))          # angles 20, 21 are copied through


def test_zero_weight_hides_a_landmark(rec00):
    r = rec00
    rows, tips = np.arange(738), np.arange(738) % 5
    w = np.ones((738, 21), np.float32)
    w[rows, tips] = 0
    hidden = r["targets"].copy()
    hidden[rows, tips] = np.nan
    ja, xf, info = _fit(r["blob"], hidden, r["hand"], weights=w)
    assert np.isfinite(ja).all() and np.isfinite(xf).all() and np.isfinite(info).all()
    err = _dist(_fk64(r["hm"], ja, xf, r["hand"]), r["targets"])[w > 0].max()
    print(f"one fingertip hidden per pose: kept landmarks {err:.3e} mm, iterations max {int(info[:, 2].max())}, status counts "
          f"{np.bincount(info[:, 3].astype(int))}")
    assert err <= KP_TOL_MM
    distal = ja[rows, 4 * tips + 3]
    assert np.array_equal(distal.view(np.uint32), np.zeros(738, np.uint32))      # the cold start's 0, bit for bit
    garbage = r["targets"].copy()
    garbage[rows, tips] = 12345.0
    ja2, xf2, info2 = _fit(r["blob"], garbage, r["hand"], weights=w)
    assert np.array_equal(ja2.view(np.uint32), ja.view(np.uint32)) and np.array_equal(xf2.view(np.uint32), xf.view(np.uint32))
    assert np.array_equal(info2, info)


def test_noisy_targets(rec00):
    """2 mm Gaussian noise on every coordinate, every third pose, started from the labels.  The rms residual of the GPU's
    pose (float64 FK against the noisy targets) is the float64 solver's within 1e-3 mm on both sides, and not above the
    start's."""
    r = rec00
    sel = np.arange(0, 738, 3)
    rng = np.random.default_rng(5)
    noisy = (r["targets"][sel] + rng.normal(0, 2.0, (len(sel), 21, 3))).astype(np.float32).astype(np.float64)
    init = (r["ja"][sel], r["xf"][sel])
    ja, xf, info = _fit(r["blob"], noisy, r["hand"][sel], init=init)
    ja64, xf64, info64 = fc.fit(r["hm"], noisy, init=init, mirror=r["hand"][sel])

    def rms(ja_, xf_):
        return np.sqrt((_dist(_fk64(r["hm"], ja_, xf_, r["hand"][sel]), noisy) ** 2).mean(1))
    got, want, start = rms(ja, xf), rms(ja64, xf64), rms(*init)
    print(f"noisy targets, {len(sel)} poses: rms residual GPU median {np.median(got):.4f} max {got.max():.4f} mm; float64 "
          f"solver median {np.median(want):.4f} max {want.max():.4f} mm; largest difference {np.abs(got - want).max():.3e} mm; "
          f"start median {np.median(start):.4f} mm; iterations GPU mean {info[:, 2].mean():.2f} max {int(info[:, 2].max())}, float64 "
          f"mean {info64[:, 2].mean():.2f} max {int(info64[:, 2].max())}; GPU status counts {np.bincount(info[:, 3].astype(int))}")
    assert np.abs(got - want).max() <= KP_TOL_MM
    assert np.all(got <= start)
    assert np.abs(info[:, 0] - got).max() <= KP_TOL_MM                    # the kernel reports the residual it reached


def test_limits(rec00):
    """With the box every output angle lies inside joint_limits, exactly; the poses whose labels lie inside are recovered
    to the bounds of the exact-target test.  For the others: finite, inside, and not worse than the start - the start
    being the rest pose clamped to the box and Kabsch-aligned, restated in float64 by fit_cases.cold_start; the kernel
    decides on float32 costs, whose forward function is off by ~3e-5 mm on residuals of millimetres, so 'not above' is
    asserted to a relative 1e-5."""
    r = rec00
    lo, hi = r["limits"][:, 0], r["limits"][:, 1]
    ja, xf, info = _fit(r["blob"], r["targets"], r["hand"], limits=r["limits"][None])
    assert np.isfinite(ja).all() and np.isfinite(xf).all()
    assert np.all(ja[:, :20] >= lo) and np.all(ja[:, :20] <= hi)
    inside = np.all((r["ja"][:, :20] >= lo) & (r["ja"][:, :20] <= hi), axis=1)
    print(f"limits: {inside.sum()} of 738 label poses inside the box; status counts of those "
          f"{np.bincount(info[inside, 3].astype(int))}, of the others {np.bincount(info[~inside, 3].astype(int))}")
    assert inside.sum() >= 300
    _check_recovered(r, np.nonzero(inside)[0], ja[inside], xf[inside], "label poses inside the box, cold start with limits")
    box = np.broadcast_to(r["limits"].astype(np.float64), (738, 20, 2))
    ang0, m0 = fc.cold_start(r["hm"], r["targets"], np.ones((738, 21)), r["hand"], box)
    start = np.sqrt((_dist(fc.forward(r["hm"], ang0, m0), r["targets"]) ** 2).mean(1))
    end = np.sqrt((_dist(_fk64(r["hm"], ja, xf, r["hand"]), r["targets"]) ** 2).mean(1))
    print(f"outside the box: rms residual start median {np.median(start[~inside]):.2f} mm, end median "
          f"{np.median(end[~inside]):.3f} max {end[~inside].max():.3f} mm")
    assert np.all(end <= start * (1 + 1e-5))


def test_shapes_and_plumbing(rec00):
    r = rec00
    whole = [torch.from_numpy(a) for a in r["got"]]
    # a pose alone, in a small batch, in a batch that does not fill its last workgroup (4 poses each), in half the set and
    # in the whole set: the same bits
    for sel in (np.array([11]), np.arange(5), np.arange(300, 307), np.arange(369)):
        ja, xf, info = _fit(r["blob"], r["targets"][sel], r["hand"][sel])
        for got, want in zip((ja, xf, info), whole):
            assert torch.equal(torch.from_numpy(got), want[sel]), len(sel)
    # one skeleton per pose
    sel = np.arange(0, 738, 41)[:10]
    factors = np.where(np.arange(len(sel)) % 2 == 0, 0.8, 1.1)
    hmt = hand.scaled_hand_model(pipeline.hand_model_from_labels(pipeline.load_labels()), torch.from_numpy(factors).float())
    hms = {k: getattr(hmt, k).numpy() for k in ("joint_rest_positions", "landmark_rest_positions")}
    for k in ("joint_rotation_axes", "landmark_rest_bone_weights", "landmark_rest_bone_indices"):
        hms[k] = np.broadcast_to(r["hm"][k], (len(sel),) + r["hm"][k].shape)
    assert hms["joint_rest_positions"].shape == (len(sel), 22, 3)
    targets = fc.forward(hms, r["ja"][sel], fc.effective_wrist(r["xf"][sel], r["hand"][sel], 1.0, np.float64))
    assert _dist(targets, r["targets"][sel]).max() > 1.0
    ja, xf, info = _fit(_blob(hms), targets, r["hand"][sel])
    err = _dist(_fk64(hms, ja, xf, r["hand"][sel]), targets).max()
    print(f"scaled skeletons (0.8 / 1.1), one model row per pose: {err:.3e} mm")
    assert _blob(hms).shape == (len(sel), 321) and err <= KP_TOL_MM and np.all(info[:, 3] == _native.UT_FIT_CONVERGED)
    assert fc.angle_distance(ja[:, :20], r["ja"][sel, :20]).max() <= ANGLE_TOL_RAD
    # outputs in place in [n,60] records: angles in columns 0..21, the wrist in 22..37, the rest untouched
    sel = np.arange(20, 27)
    rec = torch.full((len(sel), 60), 7.0, device=DEV)
    info_t = torch.empty(len(sel), 4, device=DEV)
    _native.fit_pose(r["blob"], _t(r["targets"][sel]).reshape(-1, 63), mirror=_t(r["hand"][sel], torch.int64), n=len(sel),
                     out=(rec, rec[:, 22:]), ja_stride=60, xf_stride=60, info=info_t)
    rec = rec.cpu()
    assert torch.equal(rec[:, :22], whole[0][sel]) and torch.equal(rec[:, 22:38].reshape(-1, 4, 4), whole[1][sel])
    assert torch.equal(rec[:, 38:], torch.full((len(sel), 22), 7.0)) and torch.equal(info_t.cpu(), whole[2][sel])
    # t_scale = 1000: the translation comes back in metres and ut_fk with the same t_scale round-trips
    ja, xf, info = _fit(r["blob"], r["targets"][sel], r["hand"][sel], t_scale=1000.0)
    assert np.abs(xf[:, :3, 3] * 1000 - whole[1][sel][:, :3, 3].numpy()).max() <= 1e-3
    assert _dist(_fk_gpu(r["blob"], ja, xf, r["hand"][sel], t_scale=1000.0), r["targets"][sel]).max() <= KP_TOL_MM
    assert np.array_equal(ja, whole[0][sel].numpy()) and np.array_equal(xf[:, :3, :3], whole[1][sel][:, :3, :3].numpy())
    # a refused pose (two weighted landmarks) says so, gives the rest pose at the identity and leaves its neighbours alone
    w = np.ones((len(sel), 21), np.float32)
    w[3] = 0
    w[3, [0, 5]] = 1
    ja, xf, info = _fit(r["blob"], r["targets"][sel], r["hand"][sel], weights=w)
    assert int(info[3, 3]) == _native.UT_FIT_REFUSED and np.array_equal(ja[3], np.zeros(22, np.float32))
    assert np.array_equal(xf[3], np.eye(4, dtype=np.float32)) and np.array_equal(info[3, :3], np.zeros(3, np.float32))
    keep = np.arange(len(sel)) != 3
    for got, want in zip((ja, xf, info), whole):
        assert torch.equal(torch.from_numpy(got[keep]), want[sel][keep])
    # a warm start that is refused gives its start back
    ja, xf, info = _fit(r["blob"], r["targets"][sel], r["hand"][sel], weights=w, init=(r["ja"][sel], r["xf"][sel]))
    assert int(info[3, 3]) == _native.UT_FIT_REFUSED and np.array_equal(ja[3], r["ja"][sel][3].astype(np.float32))
    assert np.array_equal(xf[3], r["xf"][sel][3].astype(np.float32))
    # the binding refuses what the entry refuses
    with pytest.raises(ValueError, match="ut_fit_pose"):
        _fit(r["blob"], r["targets"][sel], r["hand"][sel], max_iters=0)
    with pytest.raises(ValueError):
        _native.fit_pose(r["blob"], _t(r["targets"][sel]), init_angles=_t(r["ja"][sel]))


def test_wrist_is_rigid(rec00):
    """Up to 32 float32 rotation products, each off by a few 6e-8: |R^T R - I| <= 1e-5, and a proper rotation for both hands
    (the mirror is the consumer's)."""
    r = rec00
    rng = np.random.default_rng(8)
    ja0 = r["ja"].copy()
    ja0[:, :20] += rng.uniform(-0.4, 0.4, (738, 20))
    warm = _fit(r["blob"], r["targets"] + rng.normal(0, 2.0, r["targets"].shape), r["hand"], init=(ja0, r["xf"]))
    for what, (ja, xf, info) in (("cold start", r["got"]), ("warm start, noisy targets, 32 iterations", warm)):
        rot = xf[:, :3, :3].astype(np.float64)
        off = np.abs(rot.transpose(0, 2, 1) @ rot - np.eye(3)).max()
        det = np.linalg.det(rot)
        print(f"{what}: |R^T R - I| {off:.3e}, det in [{det.min():.7f}, {det.max():.7f}], iterations max {int(info[:, 2].max())}")
        assert off <= 1e-5
        assert np.all(det[r["hand"] == 0] > 0) and np.all(det[r["hand"] == 1] > 0)


def test_python_surface(rec00, golden_dir):
    r = rec00
    hmt = pipeline.hand_model_from_labels(pipeline.load_labels())
    for i in (100, 101):                                                    # a left and a right hand
        hand_idx = int(r["hand"][i])
        kp = r["targets"][i].astype(np.float32)
        pose = tracker.hand_pose_from_landmarks(hmt, kp, hand_idx)
        assert pose.joint_angles.shape == (22,) and pose.wrist_xform.shape == (4, 4) and pose.hand_confidence == 1.0
        assert np.abs(tracker.landmarks_from_hand_pose(hmt, pose, hand_idx) - kp).max() <= KP_TOL_MM
        again = tracker.hand_pose_from_landmarks(hmt, kp, hand_idx, init=pose)
        assert np.abs(tracker.landmarks_from_hand_pose(hmt, again, hand_idx) - kp).max() <= KP_TOL_MM
    # hand.fit_landmarks: leading dims, CPU tensors in and out, limits from the model
    sel = np.arange(6).reshape(2, 3)
    ja, xf, info = hand.fit_landmarks(hmt, torch.from_numpy(r["targets"][sel]).float(), mirror=torch.from_numpy(r["hand"][sel]))
    assert ja.shape == (2, 3, 22) and xf.shape == (2, 3, 4, 4) and info.shape == (2, 3, 4) and ja.device.type == "cpu"
    assert torch.equal(ja.reshape(6, 22), torch.from_numpy(r["got"][0][:6]))
    boxed = hand.fit_landmarks(hmt, torch.from_numpy(r["targets"][sel]).float(), mirror=torch.from_numpy(r["hand"][sel]), limits=True)[0]
    lim = hmt.joint_limits[:20].float()
    assert bool(((boxed[..., :20] >= lim[:, 0]) & (boxed[..., :20] <= lim[:, 1])).all())
    # a sequence in the layout of the eval result files, with its own skeleton
    g = np.load(os.path.join(golden_dir, "fk_user05.npz"))
    hm00 = pipeline.hand_model_from_labels({k[len("r00."):]: g[k] for k in g.files if k.startswith("r00.hm.")})
    kp, valid = g["r00.gt_keypoints"], g["r00.valid_tracking"]
    assert not valid.all() and valid.any()
    poses = tracker.hand_poses_from_keypoints(hm00, kp, valid)
    assert len(poses) == valid.shape[1]
    worst = 0.0
    for t, frame in enumerate(poses):
        assert sorted(frame) == [h for h in range(2) if valid[h, t]]        # invalid frames are skipped
        for h, pose in frame.items():
            worst = max(worst, float(np.abs(tracker.landmarks_from_hand_pose(hm00, pose, h) - kp[h, t]).max()))
    print(f"hand_poses_from_keypoints, recording 00: {int(valid.sum())} poses, landmarks back within {worst:.3e} mm")
    assert worst <= KP_TOL_MM


# ----------------------------------------------------------------------------- what the four fit entries refuse, word for word
N_MSG = 2                    # two poses: the smallest batch that tells "batch mismatch" from "one row"
STRIDED = "strided views must be fp32 on cuda:0, and `out` must be given with them"
STRIDED_VIEWS = "strided views must be fp32 on cuda:0, n the windows' batch, and `out` must be given with them"
NO_COLD_START = "init_angles and init_wrist_xf are required: ut_fit_pose_views has no cold start"
# fault: (what it changes in the arguments, exception, message - one for all entries, or {entry: message})
BINDING_FAULTS = {
    "init_pair": (dict(init_wrist_xf=None), ValueError, dict(fit="init_angles and init_wrist_xf go together",
                  info="init_angles and init_wrist_xf go together", scale="init_angles and init_wrist_xf go together", views=NO_COLD_START)),
    "init_batch": (dict(init_angles=(N_MSG + 1, 22)), ValueError, "init_angles / init_wrist_xf batch mismatch"),
    "mirror_batch": (dict(mirror=(N_MSG + 1,)), ValueError, "mirror batch mismatch"),
    "limits_rows": (dict(limits=(2, 20, 2)), ValueError, "limits has 2 rows for 1 model rows"),
    "model_rows": (dict(hand_model=(3, 321)), ValueError, "hand_model has 3 rows for 2 poses"),
    "strided_without_out": (dict(n=N_MSG), ValueError, dict(fit=STRIDED, info=STRIDED, scale=STRIDED, views=STRIDED_VIEWS)),
    "strided_fp16": (dict(n=N_MSG, out="fp16"), ValueError, dict(fit=STRIDED, info=STRIDED, scale=STRIDED, views=STRIDED_VIEWS)),
    "own_shape": (dict(own=True), ValueError, dict(fit="weights must be [2,21], got (2, 20)", info="sqrt_info must be [2,21,6], got (2, 21, 5)",
                  scale="init_scale batch mismatch", views="weights must be f32 [2,2,21], got torch.float32 (2, 2, 20)")),
    "scale_weights": (dict(weights=(N_MSG, 20)), ValueError, dict(scale="weights must be [2,21], got (2, 20)")),
    "no_sqrt_info": (dict(sqrt_info=None), ValueError, dict(info="sqrt_info is required")),
    "no_init": (dict(init_angles=None, init_wrist_xf=None), ValueError, dict(views=NO_COLD_START)),
    "no_views": (dict(window=(N_MSG, 0, 21, 2), cam_rows=(N_MSG, 0)), ValueError, dict(views="window [n,V,21,2] needs 1 <= V <= 8, got V = 0")),
    "f32_window": (dict(window=torch.float32), ValueError, dict(views="window must be f64 [n,V,21,2], got torch.float32 (2, 2, 21, 2)")),
    "table_31": (dict(table=(4, 31)), ValueError,
                 dict(views="table must be f64 [R,32] source cameras or [R,24] crop cameras, got torch.float64 (4, 31)")),
    "i64_cam_rows": (dict(cam_rows=torch.int64), ValueError, dict(views="cam_rows must be i32 [2,2], got torch.int64 (2, 2)")),
}
BINDING_CASES = [(e, f) for f, (_c, _x, m) in BINDING_FAULTS.items() for e in ("fit", "info", "scale", "views")
                 if not isinstance(m, dict) or e in m]


def _binding_args(entry):
    """Valid arguments of one _native entry for N_MSG poses, warm start included: every check passes, nothing is launched yet."""
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    kw = dict(hand_model=z(1, 321), init_angles=z(N_MSG, 22), init_wrist_xf=z(N_MSG, 4, 4), mirror=z(N_MSG, dtype=torch.int64),
              limits=z(1, 20, 2))
    if entry == "views":
        kw.update(window=z(N_MSG, 2, 21, 2, dtype=torch.float64), cam_rows=z(N_MSG, 2, dtype=torch.int32),
                  table=z(4, 32, dtype=torch.float64), weights=z(N_MSG, 2, 21))
    else:
        kw.update(targets=z(N_MSG, 21, 3))
    if entry == "info":
        kw.update(sqrt_info=z(N_MSG, 21, 6))
    elif entry in ("fit", "scale"):
        kw.update(weights=z(N_MSG, 21))
    if entry == "scale":
        kw.update(init_scale=z(N_MSG))
    return kw


@pytest.mark.parametrize("entry,fault", BINDING_CASES, ids=[f"{e}-{f}" for e, f in BINDING_CASES])
def test_binding_refusals_word_for_word(entry, fault):
    """One fault at a time in otherwise valid arguments of _native.fit_pose / fit_pose_info / fit_pose_scale / fit_pose_views:
    the exception's type and its whole message.  Every one of these checks raises before anything is launched."""
    change, exc, msg = BINDING_FAULTS[fault]
    msg = msg[entry] if isinstance(msg, dict) else msg
    kw = _binding_args(entry)
    for k, v in change.items():
        if k == "own":
            own = dict(fit=("weights", (N_MSG, 20)), info=("sqrt_info", (N_MSG, 21, 5)), scale=("init_scale", (N_MSG + 1,)),
                       views=("weights", (N_MSG, 2, 20)))[entry]
            kw[own[0]] = torch.zeros(own[1], device=DEV)
        elif k == "out":
            kw["out"] = (torch.zeros(N_MSG, 22, dtype=torch.float16, device=DEV), torch.zeros(N_MSG, 4, 4, device=DEV))
        elif isinstance(v, tuple):
            kw[k] = torch.zeros(v, dtype=kw[k].dtype, device=DEV)
        elif isinstance(v, torch.dtype):
            kw[k] = kw[k].to(v)
        else:
            kw[k] = v
    fn = dict(fit=_native.fit_pose, info=_native.fit_pose_info, scale=_native.fit_pose_scale, views=_native.fit_pose_views)[entry]
    with pytest.raises(exc) as e:
        fn(**kw)
    assert type(e.value) is exc and str(e.value) == msg


WRAPPER_FAULTS = {
    "leading_dims": (AssertionError, "Leading dimensions do not match, got (2,) and (3,)"),
    "no_limits": (ValueError, dict(fit="limits=True needs hand_model.joint_limits", info="limits=True needs hand_model.joint_limits",
                                   scale="limits=True needs hand_model.joint_limits", views="limits needs hand_model.joint_limits")),
    "sqrt_info_shape": (ValueError, dict(info="sqrt_info must be (2, 21, 6), got (2, 21, 5)")),
    "no_init": (ValueError, dict(views="init = (joint_angles, wrist_transforms) is required: fit_landmarks_views has no cold start")),
    "scalar_weights": (RuntimeError, dict(fit="shape '[2, 21]' is invalid for input of size 1")),
}
WRAPPER_CASES = [(e, f) for f, (_x, m) in WRAPPER_FAULTS.items() for e in ("fit", "info", "scale", "views")
                 if not isinstance(m, dict) or e in m]


@pytest.mark.parametrize("entry,fault", WRAPPER_CASES, ids=[f"{e}-{f}" for e, f in WRAPPER_CASES])
def test_wrapper_refusals_word_for_word(entry, fault):
    """hand.fit_landmarks / _info / _scale / _views on CPU tensors of N_MSG poses with one fault: the exception's type and its
    whole message.  A scalar `weights` is refused by fit_landmarks (fit_landmarks_scale alone broadcasts)."""
    exc, msg = WRAPPER_FAULTS[fault]
    msg = msg[entry] if isinstance(msg, dict) else msg
    hmt = pipeline.hand_model_from_labels(pipeline.load_labels())
    assert hmt.joint_limits is not None and hmt.joint_rest_positions.dim() == 2
    init = (torch.zeros(N_MSG, 22), torch.eye(4).repeat(N_MSG, 1, 1))
    if entry == "views":
        args = [torch.zeros(N_MSG, 2, 21, 2, dtype=torch.float64), torch.zeros(N_MSG, 2, dtype=torch.int32),
                torch.zeros(4, 32, dtype=torch.float64), init]
    else:
        args = [torch.zeros(N_MSG, 21, 3)] + ([torch.zeros(N_MSG, 21, 6)] if entry == "info" else [])
    kw = {}
    if fault == "leading_dims":
        hmt = hand.scaled_hand_model(hmt, torch.ones(3))
    elif fault == "no_limits":
        hmt, kw = hmt._replace(joint_limits=None), dict(limits=True)
    elif fault == "sqrt_info_shape":
        args[1] = torch.zeros(N_MSG, 21, 5)
    elif fault == "no_init":
        args[3] = None
    else:
        kw = dict(weights=torch.tensor(1.0))
    fn = dict(fit=hand.fit_landmarks, info=hand.fit_landmarks_info, scale=hand.fit_landmarks_scale, views=hand.fit_landmarks_views)[entry]
    with pytest.raises(exc) as e:
        fn(hmt, *args, **kw)
    assert type(e.value) is exc and str(e.value) == msg
