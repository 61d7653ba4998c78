"""GPU tests of the split-fp16 arithmetic with calibrated activation scales (include/umetrack_hip.h: UT_CONV_SPLIT_F16,
UT_SPLIT_SCALE_CALIBRATED) against the float64 oracle, across the range the calibrated words are meant for and past it.

Errors are relative to the fp64 reference's largest magnitude, with no floor at 1: a dim input is held to the same relative
bound as a bright one.  The property every call is held to: it either raises "range check" at the next status read or is within
tolerance of fp64.  Measured maxima on the MI355X are in the docstrings; tolerances are about 4 x those."""
import math

import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, pipeline, synth
from oracle import ref_model, scenarios

from head_cases import ANGLE_TOL, FP32_TOL, METRE_TOL, RAW_TOL, decode_errors, head_oracle as _head_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND_TOL = 3e-6          # relative error inside the calibrated band, 2^-7 .. the guard, every kernel selection (max seen 1.56e-6)
FLOOR_F = 2.0 ** -7      # below this fraction of the calibration maximum the split's error is absolute (the header's floor)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sd64(sd):
    return {k: v.double() for k, v in ref_model.to_torch_state_dict(sd).items()}


def _rel(got, want):
    want = torch.as_tensor(want, dtype=torch.float64)
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


def _raises(eng):
    try:
        eng.poll_status()
    except FloatingPointError as e:
        assert "range check" in str(e)
        return True
    return False


def _guard(word):
    """The largest ratio (this call's max / calibration max) a consumer of a tensor with calibrated word `word` admits:
    ut_kernels.h::split_act_scale passes an input while its exponent plus k stays <= 142 (k puts the word in [2^14, 2^15)), i.e.
    below 2^(16 - k); the word holds 2^4 x the calibration maximum.  In (32, 64] for every word."""
    e = int(np.float32(word).view(np.uint32)) >> 23
    return 2.0 ** (e - 125) / (float(word) / 16.0)


@pytest.fixture(scope="module")
def zero_bias():
    sd = synth.zero_bias_state_dict(synth.synthetic_state_dict(0))
    crops = synth.synthetic_crops(16, seed=31)
    ref = ref_model.backbone(_sd64(sd), torch.from_numpy(crops).double())
    return sd, crops, ref


SWEEP = [2.0 ** j for j in range(-24, 7)] + [3.0, 24.0, 31.0, 40.0]


def _sweep(eng, crops, ref, fs, calibrated=True):
    """[(f, raised, err)] with err = max |out - f ref| / max |f ref| (None when the call raised)."""
    out = []
    for f in fs:
        got = eng.backbone(_dev(crops * np.float32(f)))
        if _raises(eng):
            out.append((f, True, None))
        else:
            out.append((f, False, _rel(got, ref * f)))
    return out


def _check_sweep(res, band_tol, floor):
    for f, raised, err in res:
        if raised:
            continue
        if f >= FLOOR_F or not floor:
            assert err < band_tol, (f, err)
        else:       # below the band: absolute, the error the band allows at FLOOR_F of the calibration maximum
            assert err * f < band_tol * FLOOR_F, (f, err)


@pytest.mark.parametrize("resident,fusion", [(1, True), (0, True), (6, True), (1, False)])
def test_split_calibrated_magnitude_sweep_against_fp64(zero_bias, resident, fusion):
    """Zero-bias network (every tensor scales with the crops), calibrated on 16 crops C, then backbone(f C) for f = 2^-24 .. 2^6
    and f in {3, 24, 31, 40}: each call raises "range check" or is within BAND_TOL of f ref64(C) - relative from 2^-7 to the
    guard, absolute (BAND_TOL x 2^-7 of the reference at f = 1) below.  f <= 16 never raises, f = 64 always does (the stem's
    output, an exact fp32 tensor, is then 4 x its word), and a non-power-of-two f just below the smallest guard of the calibrated
    words does not.  Measured on the MI355X (guard 32.4; f = 40 and 64 raise):
      in the band, 2^-7 .. 32.25: at most 1.09e-6 (resident 1), 1.15e-6 (resident 0), 1.07e-6 (resident 6), 9.7e-7 (two-launch
        layer1);
      below it the error is absolute, |err| / max|ref(f = 1)| = 3.9e-9 at every f from 2^-9 down to 2^-24 with the fused layer1
        blocks (relative 6.6e-2 at 2^-24), 2.0e-10 with the two-launch form: the fused block scales its intermediate by an L1 bound
        of it (conv_block32.hip), tens above its calibrated maximum, and so drops the second fp16 piece ~2^4 earlier."""
    sd, crops, ref = zero_bias
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16_always")
        eng.set_resident_weights(resident)
        eng.set_block_fusion(fusion)
        eng.calibrate_split(_dev(crops))
        words = eng.split_calibration()
        guard = min(_guard(w) for w in words[:24] if w > 0)
        assert 32.0 < guard <= 64.0
        f_safe = math.floor(guard * 0.999 * 8) / 8
        res = _sweep(eng, crops, ref, SWEEP + [f_safe])
        print(f"\nsweep resident={resident} fusion={fusion} guard={guard:.4f}:",
              " ".join(f"{f:g}:{'R' if r else f'{e:.2e}'}" for f, r, e in res))
        _check_sweep(res, BAND_TOL, floor=True)
        by_f = {f: r for f, r, _e in res}
        assert not any(r for f, r in by_f.items() if f <= 16.0)
        assert by_f[64.0] and not by_f[f_safe]
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ["fp32", "dynamic"])
def test_split_sweep_controls_hold_the_relative_bound_everywhere(zero_bias, mode):
    """The same sweep with exact fp32 convolutions, and with split-fp16 on dynamic scales: no call raises and every f, down to
    2^-24, is within the band's RELATIVE tolerance - the reference is right, and what the calibrated sweep loses below the band
    is the calibrated scale's.  Measured on the MI355X: fp32 2.23e-6 at every f (the fp32 chain's own rounding, exactly homogeneous),
    dynamic 8.9e-7."""
    sd, crops, ref = zero_bias
    eng = _native.HipEngine(sd, DEV)
    try:
        if mode == "dynamic":
            eng.set_split_scale("dynamic")
            eng.set_conv_arithmetic("split_f16_always")
        res = _sweep(eng, crops, ref, SWEEP)
        print(f"\ncontrol {mode}:", " ".join(f"{f:g}:{'R' if r else f'{e:.2e}'}" for f, r, e in res))
        assert not any(r for _f, r, _e in res)
        _check_sweep(res, FP32_TOL if mode == "fp32" else BAND_TOL, floor=False)
    finally:
        eng.close()


def test_split_calibrated_two_lanes_large_batch(zero_bias):
    """set_backbone_lanes(2) on 1024 crops (64 copies of C at f = 3): within the band of fp64, and every crop has the bits of the
    16-crop call - calibrated scales do not depend on the batch or the lane.  Measured on the MI355X: 1.05e-6."""
    sd, crops, ref = zero_bias
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16_always")
        eng.calibrate_split(_dev(crops))
        small = eng.backbone(_dev(crops * np.float32(3.0)))
        eng.set_backbone_lanes(2)
        big = eng.backbone(_dev(np.tile(crops * np.float32(3.0), (64, 1, 1))))
        eng.poll_status()
        err = _rel(big, (ref * 3.0).repeat(64, 1, 1, 1))
        print(f"\ntwo lanes: {err:.2e}")
        assert err < BAND_TOL
        assert torch.equal(big.view(64, 16, *big.shape[1:]), small[None].expand(64, *small.shape))
    finally:
        eng.close()


@pytest.mark.parametrize("fusion", [True, False])
def test_split_layer1_worst_case_in_the_guarded_band(fusion):
    """layer1_worst_case_state_dict: a constant crop drives layer1's intermediates to the L1 bound conv_block32.hip sizes their
    scale from.  Calibrated on constant crops at brightness b (picked so that the stem's calibrated word sits at the bottom of its
    octave: the guard admits inputs up to ~63 x the calibration maximum), then constant and near-constant crops up to the largest
    brightness the stem's guard admits (63.1 x): each call raises or is within BAND_TOL of fp64.  With the bound taken at the
    calibrated word the fused block's intermediate left fp16's range from ~33 x on with no status bit: 2.4e-5 at 36 x, 1.3e-4 at
    63 x on the MI355X.  Sized from the largest admitted input it stays at 1.56e-6 at most.  The two-launch form guards the
    intermediate with its own word: within 1.4e-6 up to 30 x, raises from 36 x."""
    sd = synth.layer1_worst_case_state_dict(synth.synthetic_state_dict(0))
    sd64 = _sd64(sd)
    taps = {}
    ref_model.backbone(sd64, torch.ones(1, 96, 96, dtype=torch.float64), taps)
    m1 = taps["stem"].max().item()
    b = 1.01 * 2.0 ** (math.ceil(math.log2(m1 / 1.01)) - 1) / m1          # sig(b m1) = 1.01, b in [0.5, 1)
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16_always")
        eng.set_block_fusion(fusion)
        eng.calibrate_split(torch.full((4, 96, 96), b, device=DEV))
        words = eng.split_calibration()
        f_top = min(_guard(words[t]) for t in (0, 2, 4)) * (1 - 2.0 ** -8)
        assert f_top > 60.0
        noise = synth.counter_uniform("worst.noise", 96 * 96).reshape(96, 96)
        res = []
        for f in (1.0, 16.0, 30.0, 36.0, 48.0, f_top):
            crops = np.stack([np.full((96, 96), b * f), b * f * (1 - 0.01 * noise)]).astype(np.float32)
            got = eng.backbone(_dev(crops))
            if _raises(eng):
                res.append((f, True, None))
                continue
            res.append((f, False, _rel(got, ref_model.backbone(sd64, torch.from_numpy(crops).double()))))
        print(f"\nworst case fusion={fusion} f_top={f_top:.3f}:", " ".join(f"{f:g}:{'R' if r else f'{e:.2e}'}" for f, r, e in res))
        for f, raised, err in res:
            assert raised or err < BAND_TOL, (f, err)
        assert not any(r for f, r, _e in res if f <= 30.0)
        if fusion:          # the fused form checks nothing but the stem's and the block outputs' words: it must not raise
            assert not any(r for _f, r, _e in res)
    finally:
        eng.close()


@pytest.mark.parametrize("known", [True, False])
def test_split_headline_configuration_against_fp64(known):
    """The benchmark's configuration: UT_CONV_SPLIT_F16 with calibrated scales, 2048 crops = 1024 two-view samples (split
    backbone from 2 x CUs crops, split regressor from 4 x CUs samples), two steps on the same slots - cold memory, then warm
    memory under moved extrinsics - with a real skeleton (recording_00's hand model, metres).  Profiling asserts that split
    launches ran in the backbone call and in the head call.  The head's outputs against the fp64 oracle head fed the GPU's own
    features, on all 1024 samples; the backbone against fp64 on 16 sampled crops; poll_status clean after every call (the head's
    calibrated words cover real skeletons and warm memory).  Pose columns 38..59 (skeleton scale, sigmas) against the oracle's
    float64 decode of the GPU's own raw, relative, bounded as in test_gpu_head_edges.py: 4 x the distance of the same decode in
    fp32 torch, floor 4 fp32 ulp.  Measured on the MI355X, both regress modes: backbone 1.15e-6; raw 3.3e-7 of its largest;
    joint angles 1.7e-6 rad; rotation entries 4.1e-7; translations 5.5e-8 m; memory 5.6e-7 of its largest; scale 7.2e-8,
    sigmas 1.16e-7 (relative; allowed 4.8e-7, the 4 ulp floor)."""
    sd = synth.synthetic_state_dict(0)
    sd64 = _sd64(sd)
    n, s = 2048, 1024
    crops = synth.synthetic_crops(n, seed=41)
    k = scenarios._intrinsics("range.K", n, 0)
    xs = [scenarios._rigid("range.X", n, 0)]
    moved = scenarios._rigid("range.dX", n, 0)
    moved[:, :3, :3] = np.eye(3, dtype=np.float32)[None] + 0.1 * (moved[:, :3, :3] - np.eye(3, dtype=np.float32)[None])
    xs.append(np.einsum("nij,njk->nik", moved.astype(np.float64), xs[0].astype(np.float64)).astype(np.float32))
    sr = torch.arange(0, n, 2)[:, None] + torch.tensor([0, 2])
    hand = torch.arange(s) % 2
    mem_idx = torch.arange(s)
    hm = pipeline.hand_model_from_labels(scenarios.labels())
    axes = hm.joint_rotation_axes.float()
    rest = (hm.joint_rest_positions * 0.001).float()
    skel = torch.stack([axes, rest])[None]
    eng = _native.HipEngine(sd, DEV)
    temporal = ref_model.TemporalState()
    d = 62 if known else 63
    try:
        eng.set_conv_arithmetic("split_f16")
        eng.profile_begin()
        feat = eng.backbone(_dev(crops))
        assert eng.profile_end_by_kind()[1][1] > 0
        eng.poll_status()
        idx = np.linspace(0, n - 1, 16).astype(int)
        bb = _rel(feat[idx], ref_model.backbone(sd64, torch.from_numpy(crops[idx]).double()))
        errs = {"backbone": bb}
        assert bb < BAND_TOL
        for step, use in enumerate((False, True)):
            x = xs[step]
            usev = torch.full((s,), use, dtype=torch.bool)
            eng.profile_begin()
            pose, raw = eng.fuse_temporal_regress(feat, _dev(k), _dev(x), sr.to(DEV), mem_idx.to(DEV), usev.to(DEV), hand.to(DEV),
                                                  s, True, skel.to(DEV) if known else None,
                                                  _native.UT_MODE_KNOWN if known else _native.UT_MODE_UNKNOWN, want_raw=True)
            assert eng.profile_end_by_kind()[1][1] > 0
            eng.poll_status()
            mem, _ext = eng.get_memory()
            o = _head_oracle(sd64, feat.cpu(), torch.from_numpy(k), torch.from_numpy(x), sr, mem_idx, usev, hand, temporal, known,
                             (axes.double(), rest.double()))
            pose, raw = pose.cpu().double(), raw.cpu().double()
            e = {"raw": _rel(raw[:, :d], o["raw"]),
                 "angle": (pose[:, :22] - o["joint_angles"]).abs().max().item(),
                 "rot": (pose[:, 22:38].reshape(-1, 4, 4)[:, :3, :3] - o["wrist_xfs"][:, :3, :3]).abs().max().item(),
                 "trans": (pose[:, 22:38].reshape(-1, 4, 4)[:, :3, 3] - o["wrist_xfs"][:, :3, 3]).abs().max().item(),
                 "mem": _rel(mem[:s], temporal.mem[:s])}
            errs[f"step{step}"] = e
            assert e["raw"] < RAW_TOL and e["angle"] < ANGLE_TOL and e["rot"] < 1e-5 and e["trans"] < METRE_TOL, e
            assert e["mem"] < BAND_TOL, e
            dec = decode_errors(pose, raw, known, hand, torch.from_numpy(x)[sr[:, 0]])
            e["decode"] = {g: dec[g] for g in ("scale", "sigmas") if g in dec}
            assert all(v["ratio"] <= 1.0 for v in e["decode"].values()), e["decode"]
        print(f"\nheadline known={known}:", errs)
    finally:
        eng.close()
