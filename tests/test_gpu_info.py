"""GPU tests of keypoints with their information (csrc/triangulate.hip through ut_triangulate_points_info, csrc/fit_info.hip
through ut_fit_pose_info, hand.fit_landmarks_info, tracker.hand_pose_from_window_keypoints(use_information=True)) against the
float64 / float32 numpy restatement of tests/info_cases.py, which tests/test_info_host.py checks.

Bounds.  The factor: 1e-6 of its point's largest entry against the float64 restatement (both are fp64 rounded once to fp32, 6e-8;
the points they are taken at agree to 1e-9 mm).  Exact targets: 1e-3 mm on landmarks and 1e-4 rad on angles, the project's
keypoint and angle tolerances.  Noisy windows: the minimum has a residual and the cost is flat along depth, so two correct
float32 solvers stop apart; the float32 and float64 restatements, both started from the same float64 isotropic pose on the
CPU, end

    0.25 px, seed 0: final cost 1.83e-5 relative apart, landmarks 0.0086 mm apart, 0 / 1 poses at max_iters (float64 / float32)
    1 px,    seed 0: final cost 4.05e-6 relative apart, landmarks 0.0314 mm apart, 2 / 1 poses at max_iters

(worst pose each), and the GPU is held to 4 times that against the float64 restatement: COST_MARGIN, KP_MARGIN_MM."""
import numpy as np
import pytest
import torch

import fit_cases as fc
import info_cases as ic
import mesh_cases as mc
import triangulate_cases as tc
from absolutetrack_amd import _native, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KP_TOL_MM, ANGLE_TOL_RAD, FACTOR_RTOL = 1e-3, 1e-4, 1e-6
COST_MARGIN = {0.25: 4 * 1.83e-5, 1.0: 4 * 4.05e-6}
KP_MARGIN_MM = {0.25: 4 * 0.0086, 1.0: 4 * 0.0314}
AT_MAX_F32 = {0.25: 1, 1.0: 1}


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"], hm["landmark_rest_positions"],
                                      hm["landmark_rest_bone_weights"], hm["landmark_rest_bone_indices"]), torch.float32).reshape(-1, 321)


def _case_args(case):
    return (_t(case["window"]), _t(case["cam_rows"], torch.int32), _t(case["table"])), \
        dict(weights=None if case.get("weights") is None else _t(case["weights"], torch.float32))


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _fit_info(blob, targets, factor, mirror, init=None, **kw):
    """ut_fit_pose_info on numpy inputs -> numpy (joint_angles [n,22], wrist [n,4,4], info [n,4])."""
    out = _native.fit_pose_info(blob, _t(targets, torch.float32), _t(factor, torch.float32), None,
                                None if init is None else _t(init[0], torch.float32), None if init is None else _t(init[1], torch.float32),
                                _t(mirror, torch.int64), **kw)
    torch.cuda.synchronize()
    return _np(out)


def _fit(blob, targets, weights, mirror):
    out = _native.fit_pose(blob, _t(targets, torch.float32), None if weights is None else _t(weights, torch.float32), mirror=_t(mirror, torch.int64))
    torch.cuda.synchronize()
    return _np(out)


def _fk(blob, ja, xf, mirror):
    return _native.fk_stateless(blob, _t(ja, torch.float32), _t(xf, torch.float32), mirror=_t(mirror, torch.int64)).cpu().numpy().astype(np.float64)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _dist(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b, axis=-1)


@pytest.fixture(scope="module")
def golden():
    g = ic.golden_hands()
    g["blob"] = _blob(g["hm"])
    return g


@pytest.fixture(scope="module")
def noisy(golden):
    """noise px -> the seed-0 windows triangulated on the GPU (points fp32, factor), the float64 isotropic pose of those
    points (CPU) and the float64 restatement's information fit started from it, shared by the tests below."""
    out = {}
    for noise in (0.25, 1.0):
        case = dict(golden, window=ic.noisy_windows(golden, noise, 0))
        args, kw = _case_args(case)
        pts32 = torch.zeros(74, 63, device=DEV)
        _p, tri, _r, factor = _native.triangulate_points_info(*args, out_f32=pts32, point_stride=63, **kw)
        torch.cuda.synchronize()
        targets, factor = pts32.cpu().numpy().reshape(74, 21, 3), factor.cpu().numpy()
        assert np.all(tri.cpu().numpy()[..., 3] == tc.CONVERGED) and np.all((factor != 0).any(-1))
        iso = fc.fit(golden["hm"], targets.astype(np.float64), mirror=golden["hand"])
        init = (iso[0].astype(np.float32), iso[1].astype(np.float32))
        want = ic.fit_info(golden["hm"], targets.astype(np.float64), factor.astype(np.float64), init=init, mirror=golden["hand"])
        out[noise] = dict(targets=targets, factor=factor, init=init, want=want)
    return out


# ----------------------------------------------------------------------------- 1. the factor
def _triangulation_cases():
    cases = [("golden", None)]
    for kind in (tc.FISHEYE62, tc.PINHOLE):
        cases += [(f"ragged-{n}-{p}-{v}-{'fisheye' if kind == tc.FISHEYE62 else 'pinhole'}", (n, p, v, kind)) for n, p, v in ((1, 1, 2), (3, 21, 2), (13, 5, 4))]
    return cases + [("decisions", "decisions")]


@pytest.mark.parametrize("name,shape", _triangulation_cases(), ids=[c[0] for c in _triangulation_cases()])
def test_triangulation_hands_out_its_factor(golden, name, shape):
    """Points, info and residual (and points_f32) are ut_triangulate_points' bit for bit; the factor is the float64
    restatement's to 1e-6 of its point's largest entry, and exactly 0 for refused and degenerate points."""
    if shape is None:
        cases = {"golden": golden}
    elif shape == "decisions":
        cases = tc.decision_cases()
    else:
        cases = {name: tc.ragged_case(*shape[:3], kind=shape[3], seed=3)}
    n_dead = 0
    for key, case in cases.items():
        args, kw = _case_args(case)
        n, _v, p = case["window"].shape[:3]
        plain32, with32 = torch.full((n, 3 * p + 2), -7.0, device=DEV), torch.full((n, 3 * p + 2), -7.0, device=DEV)
        plain = _native.triangulate_points(*args, out_f32=plain32, point_stride=3 * p + 2, **kw)
        got = _native.triangulate_points_info(*args, out_f32=with32, point_stride=3 * p + 2, **kw)
        torch.cuda.synchronize()
        assert len(got) == 4 and got[3].shape == (n, p, 6) and got[3].dtype == torch.float32
        for a, b in zip(plain + (plain32,), got[:3] + (with32,)):
            assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)), key
        want = ic.triangulate_info(case["window"], case["cam_rows"], case["table"], case.get("weights"))
        info, factor = got[1].cpu().numpy(), got[3].cpu().numpy().astype(np.float64)
        assert np.array_equal(info[..., 3], want[1][..., 3]), key
        dead = (info[..., 3].astype(int) & (tc.REFUSED | tc.DEGENERATE)) != 0
        n_dead += int(dead.sum())
        assert np.all(factor[dead] == 0) and np.all(np.isposinf(info[dead][:, 1])), key
        live = ~dead
        assert np.all((factor[live] != 0).any(-1)) and np.isfinite(factor).all(), key
        rel = np.abs(factor - want[4]).max(-1)[live] / np.abs(want[4]).max(-1)[live]
        print(f"{key}: {int(live.sum())} factors within {float(rel.max(initial=0)):.2e} of their largest entry of the restatement's, {int(dead.sum())} all zero")
        assert float(rel.max(initial=0)) <= FACTOR_RTOL, key
    if shape == "decisions":
        assert n_dead >= 21 + 21 + 1 + 1


# ----------------------------------------------------------------------------- 2. isotropic factors
def test_isotropic_factors_are_ut_fit_pose():
    """Factors sqrt(w) I, w in [0.25, 4], on 40 label poses of both hands, exact targets, cold: ut_fk of the result within 1e-3 mm
    of ut_fit_pose's with weights w and of the targets, angles within 1e-4 rad of both, all converged."""
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand_idx = mc.label_poses(lab)
    sel = np.arange(0, 738, 37)[:20]
    sel = np.concatenate([sel, sel + 1 - 2 * (sel % 2)])            # the other hand of the same frames
    assert len(sel) == 40 and (hand_idx[sel] == 0).sum() == 20
    blob, mirror = _blob(hm), hand_idx[sel]
    targets = fc.forward(hm, ja[sel, :20], fc.effective_wrist(xf[sel], mirror, 1.0, np.float64))
    w = np.random.default_rng(2).uniform(0.25, 4.0, (40, 21)).astype(np.float32)
    got = _fit_info(blob, targets, ic.isotropic(w), mirror)
    ref = _fit(blob, targets, w, mirror)
    p_got, p_ref = _fk(blob, got[0], got[1], mirror), _fk(blob, ref[0], ref[1], mirror)
    kp_t, kp_r = _dist(p_got, targets).max(), _dist(p_got, p_ref).max()
    ang_t, ang_r = fc.angle_distance(got[0][:, :20], ja[sel, :20]).max(), fc.angle_distance(got[0][:, :20], ref[0][:, :20]).max()
    print(f"sqrt(w) I, 40 poses cold: to the targets {kp_t:.2e} mm {ang_t:.2e} rad, to ut_fit_pose {kp_r:.2e} mm {ang_r:.2e} rad; iterations "
          f"max {int(got[2][:, 2].max())} (ut_fit_pose {int(ref[2][:, 2].max())})")
    assert np.all(got[2][:, 3] == _native.UT_FIT_CONVERGED) and np.all(ref[2][:, 3] == _native.UT_FIT_CONVERGED)
    assert max(kp_t, kp_r) <= KP_TOL_MM and max(ang_t, ang_r) <= ANGLE_TOL_RAD
    # the whitened rms is sqrt(sum w d^2 / 63), the worst residual Euclidean
    assert np.all(got[2][:, 1] <= KP_TOL_MM) and np.all(got[2][:, 0] <= 2 * got[2][:, 1])


# ----------------------------------------------------------------------------- 3. the golden chain
def test_golden_chain_on_exact_windows(golden):
    """Triangulation with factor -> ut_fit_pose -> ut_fit_pose_info on the reference's windows, targets read from points_f32:
    ut_fk of the result within 1e-3 mm of the reference's landmarks, angles within 1e-4 rad of the isotropic fit's, all
    converged."""
    g = golden
    args, kw = _case_args(g)
    mirror = _t(g["hand"], torch.int64)
    pts32 = torch.zeros(74, 21, 3, device=DEV)
    _p, tri, _r, factor = pipeline.triangulate_keypoints(args[0], args[2], args[1], with_information=True, out_f32=pts32, point_stride=63, **kw)
    assert len(pipeline.triangulate_keypoints(args[0], args[2], args[1], **kw)) == 3
    iso = _native.fit_pose(g["blob"], pts32, mirror=mirror)
    got = _native.fit_pose_info(g["blob"], pts32, factor, init_angles=iso[0], init_wrist_xf=iso[1], mirror=mirror)
    torch.cuda.synchronize()
    back = _native.fk_stateless(g["blob"], got[0], got[1], mirror=mirror).cpu().numpy()
    kp = _dist(back, g["landmarks"].astype(np.float64)).max()
    ang = fc.angle_distance(got[0].cpu().numpy()[:, :20], iso[0].cpu().numpy()[:, :20]).max()
    info = got[2].cpu().numpy()
    print(f"golden chain: ut_fk {kp:.2e} mm from the reference's landmarks, angles {ang:.2e} rad from the isotropic fit's, iterations max "
          f"{int(info[:, 2].max())} after {int(iso[2][:, 2].max())} isotropic, whitened rms max {info[:, 0].max():.2e} px")
    assert np.all(info[:, 3] == _native.UT_FIT_CONVERGED) and bool((iso[2][:, 3] == _native.UT_FIT_CONVERGED).all())
    assert kp <= KP_TOL_MM and ang <= ANGLE_TOL_RAD
    # hand.fit_landmarks_info without an init launches the same two fits, from host tensors with leading dims
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    ja, xf, info2 = hand.fit_landmarks_info(model, pts32.cpu().reshape(2, 37, 21, 3), factor.cpu().reshape(2, 37, 21, 6),
                                            mirror=torch.from_numpy(g["hand"]).reshape(2, 37))
    assert ja.shape == (2, 37, 22) and xf.shape == (2, 37, 4, 4) and info2.shape == (2, 37, 4) and ja.device.type == "cpu"
    assert torch.equal(ja.reshape(74, 22), got[0].cpu()) and torch.equal(xf.reshape(74, 4, 4), got[1].cpu()) and torch.equal(info2.reshape(74, 4), got[2].cpu())
    with pytest.raises(ValueError, match="sqrt_info"):
        hand.fit_landmarks_info(model, pts32.cpu(), factor.cpu()[:, :20])


# ----------------------------------------------------------------------------- 4. noisy windows
@pytest.mark.parametrize("noise", [0.25, 1.0])
def test_noisy_windows_against_the_float64_restatement(golden, noisy, noise):
    """The kernel and the float64 restatement, both started from the SAME float64 isotropic pose: final cost within
    COST_MARGIN (relative), landmarks within KP_MARGIN_MM - 4 x what separates the float32 from the float64 restatement
    (module docstring); poses at max_iters at most the float32 restatement's + 2; and the pooled landmark error against the
    reference's landmarks at most 0.75 x that of the GPU's own isotropic fit."""
    g, c = golden, noisy[noise]
    got = _fit_info(g["blob"], c["targets"], c["factor"], g["hand"], init=c["init"])
    want = c["want"]
    cost, w_cost = got[2][:, 0].astype(np.float64) ** 2, want[2][:, 0] ** 2
    d_cost = np.abs(cost / w_cost - 1).max()
    p_got = _fk(g["blob"], got[0], got[1], g["hand"])
    d_kp = _dist(p_got, ic.landmarks_of(g, want[0], want[1])).max()
    at_max = int(((got[2][:, 3].astype(int) & _native.UT_FIT_AT_MAX_ITERS) != 0).sum())
    w_at_max = int(((want[2][:, 3].astype(int) & ic.AT_MAX_ITERS) != 0).sum())
    iso = _fit(g["blob"], c["targets"], None, g["hand"])
    truth = g["landmarks"].astype(np.float64)
    e_iso = np.sqrt((_dist(_fk(g["blob"], iso[0], iso[1], g["hand"]), truth) ** 2).mean())
    e_inf = np.sqrt((_dist(p_got, truth) ** 2).mean())
    print(f"{noise} px: cost vs float64 {d_cost:.2e} relative (margin {COST_MARGIN[noise]:.2e}), landmarks {d_kp:.4f} mm (margin "
          f"{KP_MARGIN_MM[noise]:.4f}); at max_iters {at_max} (float64 {w_at_max}, float32 {AT_MAX_F32[noise]}); iterations mean "
          f"{got[2][:, 2].mean():.1f} max {int(got[2][:, 2].max())} (float64 mean {want[2][:, 2].mean():.1f}); pooled error isotropic {e_iso:.3f} mm, "
          f"information {e_inf:.3f} mm, ratio {e_inf / e_iso:.2f}")
    assert not np.any(got[2][:, 3].astype(int) & _native.UT_FIT_REFUSED) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert d_cost <= COST_MARGIN[noise] and d_kp <= KP_MARGIN_MM[noise]
    assert at_max <= AT_MAX_F32[noise] + 2
    assert e_inf <= 0.75 * e_iso
    # the residuals the kernel reports are those ut_fk gives
    r = p_got - c["targets"].astype(np.float64)
    u = ic.whiten(c["factor"].astype(np.float64), r)
    assert np.abs(np.sqrt((u * u).sum((1, 2)) / 63) / got[2][:, 0] - 1).max() <= 1e-3
    assert np.abs(np.linalg.norm(r, axis=-1).max(1) - got[2][:, 1]).max() <= KP_TOL_MM


# ----------------------------------------------------------------------------- 5. a pose's bits do not depend on its batch
def test_batch_independence(golden, noisy):
    """n = 74, n = 5 (a partial second workgroup) and n = 1 on the 1 px windows, whose trip counts differ from pose to pose:
    pose i alone is row i of both launches."""
    g, c = golden, noisy[1.0]
    run = lambda s: _fit_info(g["blob"], c["targets"][s], c["factor"][s], g["hand"][s], init=(c["init"][0][s], c["init"][1][s]))
    whole, five = run(slice(0, 74)), run(slice(0, 5))
    assert len(set(whole[2][:, 2])) > 3
    assert _same_bits(five, [a[:5] for a in whole])
    for i in (0, 3, 4, 73):
        alone = run(slice(i, i + 1))
        assert _same_bits(alone, [a[i:i + 1] for a in whole]), i
        if i < 5:
            assert _same_bits(alone, [a[i:i + 1] for a in five]), i
    cold = _fit_info(g["blob"], c["targets"], c["factor"], g["hand"])          # the C entry's cold start: finite, same rule
    assert _same_bits(_fit_info(g["blob"], c["targets"][4:5], c["factor"][4:5], g["hand"][4:5]), [a[4:5] for a in cold])
    assert np.isfinite(cold[0]).all() and np.isfinite(cold[1]).all() and np.isfinite(cold[2]).all()


# ----------------------------------------------------------------------------- 6. decisions
def test_decisions(golden, noisy):
    g, c = golden, noisy[0.25]
    n = 6
    tg, f, mirror = c["targets"][:n].copy(), c["factor"][:n].copy(), g["hand"][:n]
    init = (c["init"][0][:n], c["init"][1][:n])
    f[0, 4] = 0
    garbage = tg.copy()
    garbage[0, 4] = 123.5
    tg[0, 4] = np.nan                             # a zero factor: its NaN target is bit-equal to finite garbage
    ref = _fit_info(g["blob"], garbage, f, mirror, init=init)
    f[1, 7, 3] = np.nan                           # a NaN factor entry
    f[2] = 0
    f[2, [0, 5], 0] = 1.0                         # two used landmarks
    tg[3, 2, 1] = np.inf                          # a non-finite target of a used landmark
    f[4, 6] = [0, 0, 0, 0, 0.25, 0]               # an off-diagonal entry alone makes a landmark used
    got = _fit_info(g["blob"], tg, f, mirror, init=init)
    status = got[2][:, 3].astype(int)
    print(f"status {status}, iterations {got[2][:, 2].astype(int)}")
    assert np.array_equal(status & _native.UT_FIT_REFUSED, [0, 4, 4, 4, 0, 0])
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert _same_bits([a[0:1] for a in got], [a[0:1] for a in ref]) and _same_bits([a[5:6] for a in got], [a[5:6] for a in ref])
    refused = slice(1, 4)
    assert np.array_equal(got[0][refused], init[0][refused]) and np.array_equal(got[1][refused], init[1][refused])
    assert np.array_equal(got[2][refused], np.tile(np.float32([0, 0, 0, 4]), (3, 1)))
    cold = _fit_info(g["blob"], tg, f, mirror)    # refused on a cold start: the rest pose at the identity
    assert not cold[0][refused].any() and np.array_equal(cold[1][refused], np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)))
    want = ic.fit_info(g["hm"], tg.astype(np.float64), f.astype(np.float64), init=init, mirror=mirror)
    assert np.array_equal(want[2][:, 3].astype(int) & ic.REFUSED, status & _native.UT_FIT_REFUSED)
    with pytest.raises(ValueError, match="sqrt_info"):
        _native.fit_pose_info(g["blob"], _t(tg), _t(f)[:, :20], mirror=_t(mirror, torch.int64))


# ----------------------------------------------------------------------------- 7. in place
def test_records_in_place(golden, noisy):
    """Rows of 128 floats: 22 angles | 16 wrist floats | 63 keypoints | padding.  The triangulation writes the keypoints
    into the rows (points_f32 with a record stride), both fits read them there and write their poses into the rows - the
    information fit into the buffers it starts from: the bits of the packed calls."""
    g = golden
    case = dict(g, window=ic.noisy_windows(g, 0.25, 0))
    args, kw = _case_args(case)
    mirror = _t(g["hand"], torch.int64)
    rec = torch.full((74, 128), -7.0, device=DEV)
    ja, xf, kp = rec[:, 0:], rec[:, 22:], rec[:, 38:]
    _p, _i, _r, factor = _native.triangulate_points_info(*args, out_f32=kp, point_stride=128, **kw)
    info_iso, info = torch.zeros(74, 4, device=DEV), torch.zeros(74, 4, device=DEV)
    _native.fit_pose(g["blob"], kp, mirror=mirror, n=74, target_stride=128, out=(ja, xf), ja_stride=128, xf_stride=128, info=info_iso)
    _native.fit_pose_info(g["blob"], kp, factor, init_angles=ja, init_wrist_xf=xf, mirror=mirror, n=74, target_stride=128,
                          init_ja_stride=128, init_xf_stride=128, out=(ja, xf), ja_stride=128, xf_stride=128, info=info)
    torch.cuda.synchronize()
    c = noisy[0.25]
    assert torch.equal(rec[:, 38:101].reshape(74, 21, 3), _t(c["targets"])) and torch.equal(factor, _t(c["factor"]))
    assert bool((rec[:, 101:] == -7).all())
    iso = _native.fit_pose(g["blob"], _t(c["targets"]), mirror=mirror)
    want = _native.fit_pose_info(g["blob"], _t(c["targets"]), _t(c["factor"]), init_angles=iso[0], init_wrist_xf=iso[1], mirror=mirror)
    torch.cuda.synchronize()
    assert torch.equal(rec[:, :22].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(rec[:, 22:38].view(torch.int32), want[1].reshape(74, 16).view(torch.int32))
    assert torch.equal(info.view(torch.int32), want[2].view(torch.int32)) and torch.equal(info_iso.view(torch.int32), iso[2].view(torch.int32))


# ----------------------------------------------------------------------------- 8. capture
def test_the_chain_is_capturable(golden):
    """Triangulation with factor (UT_CHECK_DEFERRED) -> ut_fit_pose -> ut_fit_pose_info captured in one graph and replayed:
    the bits of the eager run."""
    g = golden
    case = dict(g, window=ic.noisy_windows(g, 1.0, 0))
    args, kw = _case_args(case)
    mirror = _t(g["hand"], torch.int64)

    def buffers():
        return dict(pts=torch.zeros(74, 21, 3, dtype=torch.float64, device=DEV), tri=torch.zeros(74, 21, 4, device=DEV),
                    res=torch.zeros(74, 4, 21, device=DEV), factor=torch.zeros(74, 21, 6, device=DEV), kp=torch.zeros(74, 63, device=DEV),
                    ja=torch.zeros(74, 22, device=DEV), xf=torch.zeros(74, 4, 4, device=DEV), info=torch.zeros(74, 4, device=DEV),
                    ja2=torch.zeros(74, 22, device=DEV), xf2=torch.zeros(74, 4, 4, device=DEV), info2=torch.zeros(74, 4, device=DEV))

    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            def chain(b):
                _native.triangulate_points_info(*args, out=(b["pts"], b["tri"], b["res"], b["factor"]), out_f32=b["kp"], point_stride=63,
                                                engine=eng, **kw)
                _native.fit_pose(g["blob"], b["kp"], mirror=mirror, out=(b["ja"], b["xf"]), info=b["info"])
                _native.fit_pose_info(g["blob"], b["kp"], b["factor"], init_angles=b["ja"], init_wrist_xf=b["xf"], mirror=mirror,
                                      out=(b["ja2"], b["xf2"]), info=b["info2"])

            eager, replayed = buffers(), buffers()
            chain(eager)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                chain(replayed)
            graph.replay()
            torch.cuda.synchronize()
            eng.poll_status()
    finally:
        eng.close()
    for name in eager:
        view = torch.int64 if eager[name].dtype == torch.float64 else torch.int32
        assert torch.equal(eager[name].view(view), replayed[name].view(view)), name
    assert bool((eager["info2"][:, 2] >= 1).all()) and bool(eager["factor"].abs().sum(-1).gt(0).all())


# ----------------------------------------------------------------------------- 9. the tracker's entry
def test_hand_pose_from_window_keypoints_with_information():
    """20 label poses of both hands, exact windows of the float64 FK landmarks in the frame's four cameras:
    use_information=True gives ut_fk within 1e-3 mm of them and angles within 1e-4 rad of the labels; the default call is what
    it was - the sigma-weighted isotropic fit, bit for bit."""
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand_idx = mc.label_poses(lab)
    blob = _blob(hm)
    sel = np.arange(0, 738, 37)[:20]
    assert set(hand_idx[sel]) == {0, 1}
    hand_model = pipeline.hand_model_from_labels(lab)
    targets = fc.forward(hm, ja[sel], fc.effective_wrist(xf[sel], hand_idx[sel], 1.0, np.float64))
    worst_kp = worst_ang = 0.0
    for k, pose in enumerate(sel):
        cams = pipeline.cameras_for_frame(lab, int(pose // 2))
        table = np.stack([tracker.geometry.pack_camera_model(c) for c in cams])
        win, ez = tc.project(table[:, None], targets[k][None], tc.FISHEYE62)
        weights = ((ez > 0) & (win >= 0).all(-1) & (win[..., 0] < cams[0].width) & (win[..., 1] < cams[0].height)).astype(np.float32)
        got, info = tracker.hand_pose_from_window_keypoints(hand_model, cams, win, int(hand_idx[pose]), weights=weights, use_information=True)
        assert got.hand_confidence == 1.0 and info.shape == (21, 4) and np.all(info[:, 3] == _native.TRI_CONVERGED)
        back = _fk(blob, got.joint_angles[None], got.wrist_xform[None], hand_idx[pose:pose + 1])[0]
        worst_kp = max(worst_kp, float(_dist(back, targets[k]).max()))
        worst_ang = max(worst_ang, float(fc.angle_distance(got.joint_angles[None, :20], ja[pose:pose + 1, :20]).max()))
        if k < 3:
            pts, info3, factor = tracker.triangulate_landmarks(cams, win, weights, with_information=True)
            pts2, info2 = tracker.triangulate_landmarks(cams, win, weights)
            assert np.array_equal(pts, pts2) and np.array_equal(info3, info2) and factor.shape == (21, 6) and factor.dtype == np.float32
            plain, info_plain = tracker.hand_pose_from_window_keypoints(hand_model, cams, win, int(hand_idx[pose]), weights=weights)
            sigma = info2[:, 1].astype(np.float64)
            lw = ((sigma.min() / sigma) ** 2).astype(np.float32)
            want = tracker.fit_landmarks(hand_model, torch.from_numpy(pts2.astype(np.float32)), weights=torch.from_numpy(lw),
                                         mirror=torch.tensor(int(hand_idx[pose])))
            assert np.array_equal(plain.joint_angles, want[0].numpy()) and np.array_equal(plain.wrist_xform, want[1].numpy())
            assert np.array_equal(info_plain, info2)
            warm, _ = tracker.hand_pose_from_window_keypoints(hand_model, cams, win, int(hand_idx[pose]), weights=weights, init=plain,
                                                              use_information=True)
            assert warm.hand_confidence == 1.0 and fc.angle_distance(warm.joint_angles[None, :20], ja[pose:pose + 1, :20]).max() <= ANGLE_TOL_RAD
    print(f"window keypoints -> pose with information, 20 poses: ut_fk of the pose {worst_kp:.3e} mm, angles {worst_ang:.3e} rad")
    assert worst_kp <= KP_TOL_MM and worst_ang <= ANGLE_TOL_RAD
