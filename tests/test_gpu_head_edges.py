"""GPU tests of everything after the backbone (csrc/head.hip, the Procrustes chain of csrc/ut_math.h) against the float64 head
oracle fed the same features, at the edges the one synthetic network never reaches: all three regimes of the sigma decode, skeleton
scales over several e-folds, crafted Procrustes targets (rigid, mirrored, coplanar, near-coplanar, rank <= 1), one skeleton per
sample, FTL / temporal warps under large rotations, metre translations and focal lengths on both sides of the canonical one, and
the per-frame shape in latency mode.  Exact-fp32 convolutions unless a test says otherwise.

Engines are built from edited copies of the synthetic state dict; only the regressors' output layer
(_regressor_{k,u}._pose_regression_layers.2.{weight,bias}) is touched, and the oracle takes the same dict.
Bounds come from the references (the same computation in fp32 torch, or two float64 routes) or from the project's constants in
head_cases.py; the maxima measured on the MI355X are in the docstrings."""
import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, pipeline, synth
from oracle import ref_model, scenarios

import head_cases as hc
from head_cases import ANGLE_TOL, FP32_TOL, METRE_TOL, RAW_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# the world transform multiplies by inverse(cam0 extrinsics) before the record is rounded to fp32: undoing it in float64 returns
# the camera-space rotation with at most sqrt(3) x 1/2 fp32 ulp per entry (rows of a rotation have L1 norm <= sqrt(3)); x 4 margin
CAM_ROT_TOL = 4 * np.sqrt(3.0) * 0.5 * hc.ULP32


def _dev(a):
    return a.to(DEV) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sd64(sd):
    return {k: v.double() for k, v in ref_model.to_torch_state_dict(sd).items()}


def _rel(got, want):
    want = torch.as_tensor(want, dtype=torch.float64)
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


def _out_keys(known):
    p = f"_regressor_{'k' if known else 'u'}._pose_regression_layers.2"
    return p + ".weight", p + ".bias"


def _mode(known):
    return _native.UT_MODE_KNOWN if known else _native.UT_MODE_UNKNOWN


def _skeleton():
    hm = pipeline.hand_model_from_labels(scenarios.labels())
    return hm.joint_rotation_axes.float(), (hm.joint_rest_positions * 0.001).float()


def skeletons(rng, n):
    """n distinct skeletons: the recording's hand model scaled 0.8 .. 1.2, axes perturbed and renormalised.  (axes, rest) fp32
    [n,22,3] each."""
    axes, rest = _skeleton()
    a = axes[None].double() + 0.2 * torch.from_numpy(rng.normal(size=(n, 22, 3)))
    a = a / a.norm(dim=-1, keepdim=True)
    r = rest[None].double() * torch.from_numpy(rng.uniform(0.8, 1.2, (n, 1, 1)))
    return a.float(), r.float()


def frame(rng, views, max_angle=np.pi, max_t=2.0, focal=(50.0, 400.0), n_slots=None):
    """Descriptors of one head call: `views` = number of views per sample.  Extrinsics with rotations up to max_angle and
    translations to max_t metres (every view its own: view pairs are rotated against each other by up to pi), focal lengths
    drawn per view, alternating hand_idx, slots 0 .. S - 1."""
    views = np.asarray(views)
    n, s = int(views.sum()), len(views)
    k = np.zeros((n, 3, 3), np.float32)
    k[:, 0, 0] = k[:, 1, 1] = rng.uniform(*focal, n)
    k[:, 0, 2] = k[:, 1, 2] = 47.5
    k[:, 2, 2] = 1
    start = np.concatenate([[0], np.cumsum(views)[:-1]])
    return {"k": torch.from_numpy(k), "x": torch.from_numpy(hc.rigid4(rng, n, max_angle, max_t).astype(np.float32)),
            "sr": torch.from_numpy(np.stack([start, start + views], 1).astype(np.int64)),
            "mem": torch.arange(s), "use": torch.zeros(s, dtype=torch.bool), "hand": torch.arange(s) % 2,
            "n_slots": n_slots or s, "n": n, "s": s}


def features(rng, n, magnitude=1.0):
    return torch.from_numpy((rng.normal(size=(n, 72, 6, 6)) * magnitude).astype(np.float32))


def call(eng, feat, f, known, skel, want_raw=True):
    """One ut_fuse_temporal_regress; skel = (axes, rest) with [22,3] or [S,22,3] entries, or None."""
    sk = None
    if known:
        axes, rest = skel
        sk = torch.stack([axes, rest], -3)
        sk = _dev(sk[None] if sk.dim() == 3 else sk)
    pose, raw = eng.fuse_temporal_regress(_dev(feat), _dev(f["k"]), _dev(f["x"]), _dev(f["sr"]), _dev(f["mem"]), _dev(f["use"]),
                                          _dev(f["hand"]), f["n_slots"], bool(((f["sr"][:, 1] - f["sr"][:, 0]) == 2).all()), sk,
                                          _mode(known), want_raw=want_raw)
    eng.poll_status()
    return pose.cpu(), (raw.cpu() if want_raw else None)


def oracle(sd64, feat, f, temporal, known, skel):
    sk = tuple(t.double() for t in skel) if known else None
    return hc.head_oracle(sd64, feat, f["k"], f["x"], f["sr"], f["mem"], f["use"], f["hand"], temporal, known, sk)


def head_errors(pose, raw, o, known):
    """Errors of a pose record / raw against the oracle's outputs, in the units of the project's head tolerances."""
    pose, raw, d = pose.double(), raw.double(), 62 if known else 63
    w = pose[:, 22:38].reshape(-1, 4, 4)
    e = {"raw": _rel(raw[:, :d], o["raw"]),
         "angle": (pose[:, :22] - o["joint_angles"]).abs().max().item(),
         "rot": (w[:, :3, :3] - o["wrist_xfs"][:, :3, :3]).abs().max().item(),
         "trans": (w[:, :3, 3] - o["wrist_xfs"][:, :3, 3]).abs().max().item(),
         "sigma": ((pose[:, 39:60] - o["landmark_uncertainty_sigmas"]).abs() / o["landmark_uncertainty_sigmas"]).max().item()}
    if not known:
        e["scale"] = ((pose[:, 38] - o["skel_scales"]).abs() / o["skel_scales"]).max().item()
    return e


def mixed_views(s, known):
    """Two-view samples, every third one single-view where the mode admits them (the unknown-skeleton mode does not)."""
    return [1 if known and i % 3 == 1 else 2 for i in range(s)]


# ---------------------------------------------------------------- 2a: decode in isolation
REGIME_GAIN = 2.0


def regime_state_dict(known):
    """Output-layer rows of the sigmas (and of the skeleton scale) x 2, weight and bias: on random unit-normal features the sigma
    inputs then cover the pass-through branch (x > 20), log1p(exp(x)) on both signs and the 1e-5 clamp
    (x < -11.5); the scale's input spans several e-folds, far inside fp32 exp's range (|x| < 88)."""
    sd = dict(synth.synthetic_state_dict(0))
    wk, bk = _out_keys(known)
    w, b = sd[wk].copy(), sd[bk].copy()
    lo = 41
    w[lo:] *= np.float32(REGIME_GAIN)
    b[lo:] *= np.float32(REGIME_GAIN)
    sd[wk], sd[bk] = w, b
    return sd


@pytest.mark.parametrize("known", [True, False])
def test_decode_regimes_against_fp64_decode_of_the_same_raw(known):
    """decode_kernel against the oracle's float64 decode of the GPU's own raw (no convolution error in the comparison), 130
    samples (two full decode blocks and a ragged one) of random features, both hand_idx, 1- and 2-view samples (known-skeleton
    mode), cam0 extrinsics rotated up to pi and translated by up to 3 m, d = 62 and 63.  The test asserts the mix it needs from the
    GPU's raw: sigma inputs above 20, below -12, of both signs in between, sigma outputs equal to exactly 1e-5f, and (d = 63)
    scale inputs spanning more than 4 e-folds with exp finite.  Bound per group: 4 x the distance of the same decode in fp32 torch
    to the float64 one, floor 4 fp32 ulp of the value (head_cases.decode_errors).
    Measured on the MI355X, error (fp32-torch distance D), d = 62 / 63: sigma inputs -48.8 .. 34.4 / -39.2 .. 33.6, scale input
    -8.60 .. -0.35; angles exact; rotation entries 3.9e-8 (1.1e-6) / 6.4e-8 (1.6e-6); translations 1.3e-7 m (5.7e-7) / 1.2e-7
    (5.3e-7); sigmas 1.13e-7 (1.13e-7) / 1.09e-7 (1.09e-7) relative, scale 5.5e-8 (5.2e-8) relative - both against the 4 ulp
    floor, 4.8e-7; worst error / allowance 0.24."""
    sd = regime_state_dict(known)
    rng = np.random.default_rng(100 + known)
    s = 130
    f = frame(rng, mixed_views(s, known), max_t=3.0)
    feat = features(rng, f["n"])
    eng = _native.HipEngine(sd, DEV)
    try:
        pose, raw = call(eng, feat, f, known, _skeleton())
    finally:
        eng.close()
    d = 62 if known else 63
    x = raw[:, d - 21:d]
    assert (x > 20).any() and (x < -12).any() and ((x > 0) & (x < 20)).any() and ((x < 0) & (x > -11)).any()
    assert (pose[:, 39:60] == np.float32(1e-5)).any() and (pose[:, 39:60] >= np.float32(1e-5)).all()
    assert (raw[:, d:] == 0).all()
    if not known:
        assert raw[:, 41].max() - raw[:, 41].min() > 4.0 and raw[:, 41].abs().max() < 80.0
    else:
        assert (pose[:, 38] == 0).all()
    dec = hc.decode_errors(pose, raw, known, f["hand"], f["x"][f["sr"][:, 0]])
    print(f"\ndecode regimes known={known}: sigma inputs {x.min():.1f} .. {x.max():.1f}, scale input "
          f"{raw[:, 41].min():.2f} .. {raw[:, 41].max():.2f}:", dec)
    assert all(v["ratio"] <= 1.0 for v in dec.values()), dec


def crafted_state_dict(known, targets):
    """Output layer: zero weights, the bias's wrist slice holding `targets` [7,3]: every sample's raw is the bias."""
    sd = dict(synth.synthetic_state_dict(0))
    wk, bk = _out_keys(known)
    b = sd[bk].copy()
    b[20:41] = targets.reshape(21).astype(np.float32)
    sd[wk], sd[bk] = np.zeros_like(sd[wk]), b
    return sd


def _camera_space_rotation(pose, f):
    """out_pose[:, 22:38] with the world transform undone in float64: un-mirror right hands, multiply by cam0's extrinsics."""
    w = pose[:, 22:38].reshape(-1, 4, 4).double().clone()
    w[f["hand"] == 1, :, 0] *= -1
    return (f["x"][f["sr"][:, 0]].double() @ w).numpy()


@pytest.mark.parametrize("known", [True, False])
@pytest.mark.parametrize("family", list(hc.WELL_POSED) + list(hc.RANK_LE_1))
def test_decode_crafted_procrustes_targets(family, known):
    """One engine per target set (zero output-layer weights, the set in the bias, fp32 arithmetic: no calibration pass), 130
    samples that differ in what is per sample: hand_idx, 1-/2-view (known-skeleton mode), cam0 extrinsics with rotations up to pi
    and translations to 3 m.  raw must be the bias (to the rounding of pooling 36 equal values).
    Well-posed sets (rigid image of the source, anisotropic, mirrored on each axis, third factor +-1e-7, coplanar): the record
    against the float64 decode of the same raw at decode_errors' fp32-torch bound, and - because fp32 torch's SVD is itself
    arbitrary on a near-singular set, which makes that bound loose there - the camera-space rotation (world transform undone in
    float64) against numpy's float64 V diag(1, 1, det) U^T within CAM_ROT_TOL = 4.1e-7, the rounding of the fp32 record alone.
    This is the device build (fma contraction in the Jacobi sweeps) of what test_head_math_host.py checks on the host.
    Rank <= 1 sets (collinear, coincident, zero): properties of the camera-space rotation, as on the host but at the fp32
    record's precision: |R R^T - I| and |det R - 1| below 1e-6 (three products of entries rounded to 1/2 ulp, sqrt(3) each way),
    R u1 = v1 for the collinear set, R = I for the zero set, and the translation against the float64 decode.
    Measured on the MI355X, all sets and both modes: camera-space |R - R_ref64| at most 3.95e-8 (CAM_ROT_TOL 4.1e-7: the device
    build's float64 chain is invisible under the record's rounding); world rotation entries 3.2e-8 (fp32-torch distance 3.2e-7 ..
    1.1e-6), translations 2.4e-7 m (4.4e-7 .. 9.0e-7), worst error / allowance 0.13; rank <= 1: |R R^T - I| at most 9.2e-8,
    |det R - 1| 7.7e-8, |R u1 - v1| 3.8e-8, |R - I| 4.1e-8 for the zero set, translation 1.8e-7 m (bound 5.7e-6).  With the parent's
    kabsch_rotation the three rank <= 1 sets fail (|R R^T - I| ~ 1)."""
    idx = (list(hc.WELL_POSED) + list(hc.RANK_LE_1)).index(family)
    rng = np.random.default_rng(200 + 2 * idx + known)
    tgt = hc.collinear_fp32() if family == "collinear" else hc.targets(family, np.random.default_rng(300 + idx), 1)[0]
    sd = crafted_state_dict(known, tgt)
    s = 130
    f = frame(rng, mixed_views(s, known), max_t=3.0)
    feat = features(rng, f["n"])
    eng = _native.HipEngine(sd, DEV)
    try:
        pose, raw = call(eng, feat, f, known, _skeleton())
    finally:
        eng.close()
    d = 62 if known else 63
    bias = torch.from_numpy(sd[_out_keys(known)[1]])
    assert (raw[:, :d] - bias).abs().max() <= 2 * hc.ULP32 * bias.abs().max()      # mean of 36 equal values, then + 0
    r_cam = _camera_space_rotation(pose, f)
    dst = raw[:, 20:41].double().numpy().reshape(s, 7, 3)
    h = hc.cross_covariance(dst)
    dec = hc.decode_errors(pose, raw, known, f["hand"], f["x"][f["sr"][:, 0]])
    if family in hc.WELL_POSED:
        ra, rb, sv = hc.reference_rotation(h)
        assert np.abs(ra - rb).max() < 1e-12          # the fp32-rounded set is still well posed in float64
        cam = np.abs(r_cam[:, :3, :3] - ra).max()
        print(f"\ncrafted {family} known={known}: sv {sv[0] / sv[0, 0]}, camera-space |R - R_ref64| {cam:.2e};", dec)
        assert cam < CAM_ROT_TOL
        assert all(v["ratio"] <= 1.0 for v in dec.values()), dec
        return
    orth, det = hc.rotation_defects(r_cam[:, :3, :3])
    lead = 0.0
    if family == "collinear":
        u, sv, vt = np.linalg.svd(h)
        assert (sv[:, 1] < 1e-12 * sv[:, 0]).all()           # rank 1 as the kernel sees it: the set is exact in fp32
        lead = np.abs(np.einsum("nij,nj->ni", r_cam[:, :3, :3], u[:, :, 0]) - vt[:, 0, :]).max()
    if family == "zero":
        assert not h.any()
        lead = np.abs(r_cam[:, :3, :3] - np.eye(3)).max()
    # t = mean(dst) - R mean(src) in camera space: the decode's translation rule with the GPU's own rotation
    src = hc.source_points()
    t_want = dst.mean(1) - r_cam[:, :3, :3] @ src.mean(0)
    t_err = np.abs(r_cam[:, :3, 3] - t_want).max()
    print(f"\ncrafted {family} known={known}: |R R^T - I| {orth:.2e}, |det - 1| {det:.2e}, lead/identity {lead:.2e}, "
          f"translation {t_err:.2e};", {g: dec[g] for g in ("angles", "sigmas")})
    assert orth < 1e-6 and det < 1e-6 and lead < 1e-6
    assert t_err < 4 * 3.0 * 4 * hc.ULP32          # |t| <= 3 m x (rows' L1 norm <= 2 + translation) at 4 ulp
    assert all(dec[g]["ratio"] <= 1.0 for g in ("angles", "sigmas")), dec


# ---------------------------------------------------------------- 2b: one skeleton per sample
@pytest.mark.parametrize("s", [3, 37, 300])
def test_per_sample_skeletons_against_fp64_and_single_calls(s):
    """n_skel == n_samples with distinct skeletons (known-skeleton mode), backbone features of synthetic crops, mixed 1-/2-view
    samples: against the float64 oracle head at the head's tolerances (RAW_TOL relative, ANGLE_TOL, 1e-5 rotation entries,
    METRE_TOL - fp32 arithmetic here, so far inside them), and bit for bit against the same samples run one at a time with
    n_skel == 1 on a second engine.  A wrong skeleton stride in skeleton_kernel or temporal_out_kernel fails both.
    Measured on the MI355X, S = 3 / 37 / 300: raw 1.9e-7 / 2.6e-7 / 2.7e-7 of its largest (RAW_TOL 1.3e-6), angles 3.4e-7 / 7.1e-7 /
    8.6e-7 rad, rotation entries 5.3e-8 / 1.2e-7 / 2.2e-7, translations 7.4e-9 / 2.6e-8 / 4.1e-8 m; the neighbour's skeleton moves
    raw by 4.7e-2 .. 6.8e-2 of its largest; single calls bit-identical."""
    sd = synth.synthetic_state_dict(0)
    sd64 = _sd64(sd)
    rng = np.random.default_rng(400 + s)
    f = frame(rng, mixed_views(s, True), max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
    skel = skeletons(rng, s)
    eng, one = _native.HipEngine(sd, DEV), _native.HipEngine(sd, DEV)
    try:
        feat = eng.backbone(_dev(synth.synthetic_crops(f["n"], seed=50 + s))).cpu()
        pose, raw = call(eng, feat, f, True, skel)
        e = head_errors(pose, raw, oracle(sd64, feat, f, ref_model.TemporalState(), True, skel), True)
        # the skeleton must matter at this tolerance, or the comparison shows nothing: sample i under skeleton i + 1
        swapped = tuple(torch.roll(t, 1, 0) for t in skel)
        moved = _rel(oracle(sd64, feat, f, ref_model.TemporalState(), True, swapped)["raw"],
                     oracle(sd64, feat, f, ref_model.TemporalState(), True, skel)["raw"])
        print(f"\nper-sample skeletons S={s}:", e, f"(neighbour's skeleton moves raw by {moved:.2e})")
        assert moved > 100 * RAW_TOL
        assert e["raw"] < RAW_TOL and e["angle"] < ANGLE_TOL and e["rot"] < 1e-5 and e["trans"] < METRE_TOL, e
        for i in range(s):
            r0, r1 = f["sr"][i].tolist()
            fi = {"k": f["k"][r0:r1], "x": f["x"][r0:r1], "sr": torch.tensor([[0, r1 - r0]]), "mem": torch.tensor([0]),
                  "use": torch.zeros(1, dtype=torch.bool), "hand": f["hand"][i:i + 1], "n_slots": 1}
            p1, w1 = call(one, feat[r0:r1], fi, True, (skel[0][i], skel[1][i]))
            assert torch.equal(p1[0], pose[i]) and torch.equal(w1[0], raw[i]), i
    finally:
        eng.close()
        one.close()


def test_per_sample_skeletons_with_the_split_regressor():
    """The same with the split-fp16 regressor engaged: conv arithmetic split_f16, S = 4 x CUs two-view samples (profiling asserts
    split launches in the head call), one distinct skeleton per sample (scaled 0.8 .. 1.2), poll_status clean - the built-in
    calibration admits them - and the head's tolerances against float64.  Measured on the MI355X (S = 1024): raw 3.3e-7 of its largest, angles 1.2e-6 rad, rotation entries 2.3e-7, translations 4.0e-8 m,
    no range check raised."""
    sd = synth.synthetic_state_dict(0)
    sd64 = _sd64(sd)
    s = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(450)
    f = frame(rng, [2] * s, max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
    skel = skeletons(rng, s)
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16")
        feat = eng.backbone(_dev(synth.synthetic_crops(f["n"], seed=51))).cpu()
        eng.poll_status()
        eng.profile_begin()
        pose, raw = call(eng, feat, f, True, skel)
        assert eng.profile_end_by_kind()[1][1] > 0
        e = head_errors(pose, raw, oracle(sd64, feat, f, ref_model.TemporalState(), True, skel), True)
        print(f"\nper-sample skeletons, split regressor, S={s}:", e)
        assert e["raw"] < RAW_TOL and e["angle"] < ANGLE_TOL and e["rot"] < 1e-5 and e["trans"] < METRE_TOL, e
    finally:
        eng.close()


# ---------------------------------------------------------------- 2c: FTL and temporal warp on chosen features
@pytest.mark.parametrize("known", [True, False])
@pytest.mark.parametrize("magnitude", [2.0 ** -6, 1.0, 2.0 ** 6])
def test_ftl_and_temporal_warp_on_chosen_features(magnitude, known):
    """Features drawn directly (normal x magnitude), every view with its own extrinsics (pairs rotated up to pi against each
    other, translations to 2 m) and focal length (50 .. 400: f / 200 on both sides of 1).  Three steps on one engine and one
    oracle state: cold on slots 0 .. 5; warm on the same slots with every cam0 moved by a fresh large rotation; warm with the slots
    permuted, one sample jumping to slot 37 (the slot capacity doubles several times) and slots 1, 2 and 4 untouched.  raw and
    get_memory() (memory; prev_ext exactly) and the pose record against the float64 oracle, each relative to the oracle's largest,
    at FP32_TOL; the record also per group against the float64 decode of the GPU's own raw (decode_errors), which the Procrustes'
    conditioning on noise-like targets does not blur; untouched slots and their prev_ext bit-identical across step 3.
    Measured on the MI355X, worst of the three steps, magnitude 2^-6 / 1 / 2^6: raw 2.9e-7 / 2.7e-7 / 3.4e-7, memory 7.2e-7 /
    5.3e-7 / 4.3e-7 (FP32_TOL 5e-6), prev_ext exact, record 3.4e-7, decode error / allowance at most 0.20."""
    sd = synth.synthetic_state_dict(0)
    sd64 = _sd64(sd)
    rng = np.random.default_rng(500 + known)
    skel = _skeleton()
    temporal = ref_model.TemporalState()
    steps = []
    for step in range(3):
        views = mixed_views(6, known) if step < 2 else mixed_views(4, known)
        f = frame(rng, views, n_slots=6 if step < 2 else 38)
        if step > 0:
            f["use"] = torch.ones(f["s"], dtype=torch.bool)
        if step == 2:
            f["mem"] = torch.tensor([3, 37, 0, 5])
            f["use"] = torch.tensor([True, False, True, True])
        steps.append((f, features(rng, f["n"], magnitude)))
    eng = _native.HipEngine(sd, DEV)
    errs = []
    try:
        for step, (f, feat) in enumerate(steps):
            before = [t.cpu() for t in eng.get_memory()]
            pose, raw = call(eng, feat, f, known, skel)
            mem, ext = (t.cpu() for t in eng.get_memory())
            o = oracle(sd64, feat, f, temporal, known, skel)
            d = 62 if known else 63
            n_slots = temporal.mem.shape[0]
            assert mem.shape[0] >= n_slots
            e = {"raw": _rel(raw[:, :d], o["raw"]), "mem": _rel(mem[:n_slots], temporal.mem),
                 "ext": (ext[:n_slots].double() - temporal.prev_ext).abs().max().item()}
            dec = hc.decode_errors(pose, raw, known, f["hand"], f["x"][f["sr"][:, 0]])
            e["decode"] = {g: round(v["ratio"], 3) for g, v in dec.items()}
            e["pose"] = head_errors(pose, raw, o, known)          # per group against the full oracle: reported
            rec = torch.zeros(f["s"], 60, dtype=torch.float64)
            rec[:, :22], rec[:, 22:38], rec[:, 39:] = o["joint_angles"], o["wrist_xfs"].reshape(-1, 16), o["landmark_uncertainty_sigmas"]
            if not known:
                rec[:, 38] = o["skel_scales"]
            e["record"] = _rel(pose, rec)
            errs.append(e)
            assert e["raw"] < FP32_TOL and e["mem"] < FP32_TOL and e["record"] < FP32_TOL and e["ext"] == 0.0, (step, e)
            assert all(v["ratio"] <= 1.0 for v in dec.values()), (step, dec)
            if step == 2:
                for slot in (1, 2, 4):
                    assert torch.equal(mem[slot], before[0][slot]) and torch.equal(ext[slot], before[1][slot]), slot
                assert not mem[6:37].any() and not ext[6:37].any()
        print(f"\nftl/temporal magnitude={magnitude} known={known}:", errs)
    finally:
        eng.close()


# ---------------------------------------------------------------- 2d: the per-frame shape in latency mode
def test_latency_mode_backbone_and_head_against_fp64():
    """What HandTracker.track_frame runs: latency mode on (split-K convolutions: the fp32 sums in another order), the backbone at
    1, 2, 3 and 4 crops and the head at 1 and 2 samples with 1-/2-view mixes, against float64: backbone, raw and memory relative to
    the reference's largest at FP32_TOL with no floor at 1, the record at ANGLE_TOL / 1e-5 / METRE_TOL.  Beside each backbone
    figure the distance of the oracle run in fp32 to the same oracle in float64 - the rounding any fp32 chain has on this input.
    Measured on the MI355X, 1 / 2 / 3 / 4 crops: backbone 7.1e-7 / 8.1e-7 / 6.4e-7 / 7.9e-7 (oracle in fp32: 5.2e-7 / 5.2e-7 /
    5.4e-7 / 5.5e-7; FP32_TOL 5e-6 - no count needs more); head, worst of the five view mixes and two steps: raw 3.4e-7, memory
    7.7e-7, angles 7.2e-7 rad, rotation entries 1.2e-7, translations 2.3e-8 m."""
    sd = synth.synthetic_state_dict(0)
    sd64, sd32 = _sd64(sd), ref_model.to_torch_state_dict(sd)
    skel = _skeleton()
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_latency_mode(True)
        feats, report = {}, {}
        for n in (1, 2, 3, 4):
            crops = torch.from_numpy(synth.synthetic_crops(n, seed=60 + n))
            got = eng.backbone(_dev(crops)).cpu()
            eng.poll_status()
            want = ref_model.backbone(sd64, crops.double())
            report[f"backbone{n}"] = (_rel(got, want), _rel(ref_model.backbone(sd32, crops), want))
            feats[n] = got
        print("\nlatency mode (GPU vs fp64, oracle fp32 vs fp64):", report)
        for n in (1, 2, 3, 4):
            assert report[f"backbone{n}"][0] < FP32_TOL, report
        rng = np.random.default_rng(600)
        for views in ([1], [2], [1, 2], [2, 1], [2, 2]):
            f = frame(rng, views, max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
            feat = feats[f["n"]]
            eng.reset_memory()
            temporal = ref_model.TemporalState()
            for step in range(2):       # cold, then warm under moved extrinsics
                if step:
                    f = dict(f, x=torch.from_numpy(hc.rigid4(rng, f["n"], 1.2, 0.3).astype(np.float32)),
                             use=torch.ones(f["s"], dtype=torch.bool))
                pose, raw = call(eng, feat, f, True, skel)
                mem, _ext = (t.cpu() for t in eng.get_memory())
                o = oracle(sd64, feat, f, temporal, True, skel)
                e = head_errors(pose, raw, o, True)
                e["mem"] = _rel(mem[:f["s"]], temporal.mem)
                print(f"latency head views={views} step={step}:", e)
                assert e["raw"] < FP32_TOL and e["mem"] < FP32_TOL, (views, step, e)
                assert e["angle"] < ANGLE_TOL and e["rot"] < 1e-5 and e["trans"] < METRE_TOL, (views, step, e)
    finally:
        eng.close()
