"""GPU tests of the adaptive split-scale mode (include/umetrack_hip.h: UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE, HipEngine
.set_split_scale("adaptive")): calibrated scales in band, the dynamic mode's launch outside it, decided per launch on the device.

The fp64 harness is the one of test_gpu_split_range.py (zero-bias network, float64 oracle, errors relative to the reference's
largest magnitude with no floor); its helpers are copied here, not imported.  Contract checked:
  - no finite input raises, and every call is within the band's RELATIVE tolerance of fp64 from 2^-24 to 2^12;
  - in band the output is bit-identical to the calibrated mode's, with the calibrated mode's batch independence, and nothing
    is counted;
  - out of band the output is bit-identical to the dynamic mode's, and every adapted launch is counted once;
  - the decision is taken on the device: a replayed hipGraph adapts;
  - an infinity or a NaN still raises."""
import math

import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, pipeline, synth
from oracle import ref_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND_TOL = 3e-6          # relative error against fp64 (test_gpu_split_range.py: max seen in band 1.56e-6)
RAW_TOL = 1.3e-6         # split regressor's raw outputs, relative to the largest (test_gpu_split_range.py)
ANGLE_TOL = 1e-4         # rad, records against the exact-fp32 mode's
KP_TOL_MM = 1e-3         # mm, keypoints of the records against the exact-fp32 mode's
SWEEP = [2.0 ** j for j in range(-24, 13)] + [3.0, 24.0, 31.0, 40.0]
BRIGHT = 4096.0          # biased network: calibration on crops this much brighter puts normal frames below the band's floor


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sd64(sd):
    return {k: v.double() for k, v in ref_model.to_torch_state_dict(sd).items()}


def _rel(got, want):
    want = torch.as_tensor(want, dtype=torch.float64)
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


@pytest.fixture(scope="module")
def zero_bias():
    sd = synth.zero_bias_state_dict(synth.synthetic_state_dict(0))
    crops = synth.synthetic_crops(16, seed=31)
    ref = ref_model.backbone(_sd64(sd), torch.from_numpy(crops).double())
    return sd, crops, ref


def _split_engine(sd, crops=None, resident=1, fusion=True):
    eng = _native.HipEngine(sd, DEV)
    eng.set_conv_arithmetic("split_f16_always")
    eng.set_resident_weights(resident)
    eng.set_block_fusion(fusion)
    if crops is not None:
        eng.calibrate_split(_dev(crops))
    return eng


@pytest.mark.parametrize("resident,fusion", [(1, True), (0, True), (6, True), (1, False)])
def test_adaptive_sweep_is_relative_everywhere(zero_bias, resident, fusion):
    """Calibrated on 16 crops C, backbone(f C) for f = 2^-24 .. 2^12 and f in {3, 24, 31, 40}: no call raises and every one is
    within BAND_TOL of f ref64(C), relative, with no floor (calibrated mode: 6.6e-2 at 2^-24, and f >= 64 raises).  Nothing
    adapts from 2^-7 to 16 (inside every tensor's band); below 2^-9 and from 64 on, launches adapt."""
    sd, crops, ref = zero_bias
    eng = _split_engine(sd, crops, resident, fusion)
    try:
        eng.set_split_scale("adaptive")
        eng.split_adaptations(reset=True)
        res = []
        for f in SWEEP:
            got = eng.backbone(_dev(crops * np.float32(f)))
            eng.poll_status()
            res.append((f, _rel(got, ref * f), eng.split_adaptations(reset=True)))
        print(f"\nadaptive sweep resident={resident} fusion={fusion}:", " ".join(f"{f:g}:{e:.2e}/{n}" for f, e, n in res))
        for f, err, n in res:
            assert err < BAND_TOL, (f, err)
            if 2.0 ** -7 <= f <= 16.0:
                assert n == 0, (f, n)
            if f <= 2.0 ** -9 or f >= 64.0:
                assert n > 0, (f, n)
    finally:
        eng.close()


@pytest.mark.parametrize("fusion", [True, False])
def test_adaptive_bits_are_calibrated_in_band_and_dynamic_outside(zero_bias, fusion):
    """Same handle, same calibration.  In band (f in {2^-7, 1, 16}) the adaptive output has the calibrated mode's bits and
    counts nothing.  At f in {2^-24, 64, 4096} every launch of the zero-bias network is out of band: the output has the dynamic
    mode's bits (the fused layer1 block's intermediate bound included), and the counter holds exactly one count per split launch."""
    sd, crops, _ref = zero_bias
    eng = _split_engine(sd, crops, fusion=fusion)
    try:
        for f in (2.0 ** -7, 1.0, 16.0):
            x = _dev(crops * np.float32(f))
            eng.set_split_scale("calibrated")
            want = eng.backbone(x)
            eng.set_split_scale("adaptive")
            eng.split_adaptations(reset=True)
            got = eng.backbone(x)
            eng.poll_status()
            assert torch.equal(got, want), f
            assert eng.split_adaptations() == 0, f
        for f in (2.0 ** -24, 64.0, 4096.0):
            x = _dev(crops * np.float32(f))
            eng.set_split_scale("dynamic")
            want = eng.backbone(x)
            eng.poll_status()
            eng.set_split_scale("adaptive")
            eng.split_adaptations(reset=True)
            eng.profile_begin()
            got = eng.backbone(x)
            split_launches = eng.profile_end_by_kind()[1][1]
            eng.poll_status()
            assert torch.equal(got, want), f
            assert split_launches > 0 and eng.split_adaptations() == split_launches, f
    finally:
        eng.close()


def test_adaptive_in_band_is_batch_independent():
    """The calibrated mode's batch independence (test_gpu_parity.py, calibrated scales (i)) holds in adaptive mode on the
    built-in calibration: a crop alone, in a sub-batch, at pass size 9 and on two lanes has the same bits - the calibrated mode's
    bits - and nothing adapts."""
    crops = _dev(synth.synthetic_crops(40, seed=17))
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    two = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        eng.set_conv_arithmetic("split_f16_always")
        calibrated = eng.backbone(crops)
        eng.set_split_scale("adaptive")
        eng.split_adaptations(reset=True)
        whole = eng.backbone(crops)
        assert torch.equal(whole, calibrated)
        assert torch.equal(eng.backbone(crops[7:8]), whole[7:8])
        assert torch.equal(eng.backbone(crops[11:29]), whole[11:29])
        eng.set_backbone_chunk(9)
        assert torch.equal(eng.backbone(crops), whole)
        eng.set_backbone_chunk(0)
        eng.poll_status()
        assert eng.split_adaptations() == 0
        two.set_conv_arithmetic("split_f16_always")
        two.set_split_scale("adaptive")
        two.set_backbone_lanes(2)
        big = two.backbone(crops.repeat(26, 1, 1))          # 1040 crops: two lanes
        two.poll_status()
        assert torch.equal(big, whole.repeat(26, 1, 1, 1))
        assert two.split_adaptations() == 0
    finally:
        eng.close()
        two.close()


@pytest.fixture(scope="module")
def headline():
    """bench.py's headline shard: 1024 frames of recording_00's cameras and poses, 2048 hand-frames (4096 crops), u8 noise."""
    lab = pipeline.load_labels()
    hm = pipeline.hand_model_from_labels(lab)
    plan = {k: v.cpu().numpy() for k, v in pipeline.crop_plan_on_device(lab, hm, range(0, 1024), DEV).items()}
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    src = torch.randint(0, 256, (1024 * 4, 480, 636), dtype=torch.uint8, device=DEV, generator=gen)
    batch = pipeline.make_batch(plan, src, DEV)
    assert batch.n_samples == 2048
    return hm, batch


def _records_close(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    angle = (got[:, :22] - want[:, :22]).abs().max().item()
    kp = (got[:, 60:] - want[:, 60:]).abs().max().item()
    return angle, kp


def _bright_engine(hm):
    """Biased network calibrated on crops 4096 x brighter than normal ones.  (Calibrating on crops / 4096 does not take
    normal frames past the guard in the biased network: the biases then set the calibrated words, and the frames stay in band.)"""
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    eng.set_conv_arithmetic("split_f16")
    eng.calibrate_split(_dev(synth.synthetic_crops(64, seed=5) * np.float32(BRIGHT)))
    return eng, pipeline.HotPath(eng, hm, known_skeleton=True)


def test_adaptive_headline_step_past_the_band(headline):
    """Biased network, calibrated on crops x 4096, then the 2048-hand-frame HotPath step on normal frames, which lie below the
    band's floor: the calibrated mode's records differ from the adaptive mode's (the step reaches past the band).  The adaptive
    records are within 1e-4 rad / 1e-3 mm of the exact-fp32 mode's; launches adapted in the backbone call and in the head call
    (the split regressor runs at 1024 samples); the regressor's raw outputs on the same features are within RAW_TOL of the fp32
    regressor's."""
    hm, b = headline
    eng, hot = _bright_engine(hm)
    try:
        calibrated = hot.step(b).clone()
        hot.check()
        eng.set_conv_arithmetic("fp32")
        want = hot.step(b).clone()
        hot.check()
        eng.set_conv_arithmetic("split_f16")
        with eng.modes(split_scale="adaptive"):
            eng.split_adaptations(reset=True)
            got = hot.step(b).clone()
            hot.check()
            n_step = eng.split_adaptations(reset=True)
            angle, kp = _records_close(got, want)
            # the two calls of the step apart, and the regressor alone on the same features
            feat = eng.warp_backbone(b.src, b.cam_params, b.crop_params, b.src_index, _native.UT_REMAP_CV2_FIXED)
            eng.poll_status()
            n_backbone = eng.split_adaptations(reset=True)
            head_args = (feat, b.intrinsics, b.extrinsics, b.sample_range, b.memory_idx, b.use_memory, b.hand_idx, b.n_slots,
                         b.all_multiview, hot.skel, _native.UT_MODE_KNOWN)
            _pose, raw = eng.fuse_temporal_regress(*head_args, want_raw=True)
            raw = raw.clone()
            eng.poll_status()
            n_head = eng.split_adaptations(reset=True)
            eng.set_conv_arithmetic("fp32")
            _pose, raw32 = eng.fuse_temporal_regress(*head_args, want_raw=True)
            eng.set_conv_arithmetic("split_f16")
        raw_err = _rel(raw[:, :62], raw32[:, :62].double().cpu())
        c_angle, c_kp = _records_close(calibrated, want)
        print(f"\nheadline past the band: adapted {n_step} (backbone {n_backbone}, head {n_head}); angle {angle:.2e} rad, "
              f"keypoints {kp:.2e} mm, raw {raw_err:.2e}; calibrated mode: angle {c_angle:.2e} rad, keypoints {c_kp:.2e} mm")
        assert not torch.equal(got, calibrated)
        assert angle < ANGLE_TOL and kp < KP_TOL_MM, (angle, kp)
        assert n_backbone > 0 and n_head > 0 and n_step == n_backbone + n_head
        assert raw_err < RAW_TOL, raw_err
        assert eng.split_scale == "calibrated"
    finally:
        eng.close()


def test_adaptive_headline_step_in_band_is_the_calibrated_step(headline):
    """On the built-in calibration the headline step is in band everywhere: the adaptive mode's records are the calibrated
    mode's, bit for bit, and nothing adapts."""
    hm, b = headline
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        eng.set_conv_arithmetic("split_f16")
        hot = pipeline.HotPath(eng, hm, known_skeleton=True)
        want = hot.step(b).clone()
        hot.check()
        eng.set_split_scale("adaptive")
        eng.split_adaptations(reset=True)
        got = hot.step(b).clone()
        hot.check()
        assert torch.equal(got, want)
        assert eng.split_adaptations() == 0
    finally:
        eng.close()


def test_adaptive_decision_is_taken_inside_a_replayed_graph(headline):
    """One lane, calibrated on crops x 4096 so that normal frames are out of band: one adaptive-mode HotPath step captured into
    a hipGraph as bench.py --graph does, the counter zeroed, the graph replayed.  The replay adapts as many launches as the eager
    step did, raises nothing, and its records are within the tolerances of the eager step's against the exact-fp32 mode."""
    hm, b = headline
    eng, hot = _bright_engine(hm)
    try:
        eng.set_conv_arithmetic("fp32")
        want = hot.step(b).clone()
        hot.check()
        eng.set_conv_arithmetic("split_f16")
        eng.set_split_scale("adaptive")
        eng.split_adaptations(reset=True)
        hot.step(b)
        hot.check()
        n_eager = eng.split_adaptations(reset=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(eng.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                rec = hot.step(b)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eng.split_adaptations(reset=True)
        g.replay()
        torch.cuda.synchronize()
        n_replay = eng.split_adaptations()
        hot.check()
        angle, kp = _records_close(rec, want)
        print(f"\ngraph replay: adapted {n_replay} (eager {n_eager}); angle {angle:.2e} rad, keypoints {kp:.2e} mm")
        assert n_replay > 0 and n_replay == n_eager
        assert angle < ANGLE_TOL and kp < KP_TOL_MM, (angle, kp)
        del g
    finally:
        eng.close()


def test_adaptive_still_raises_on_an_infinity():
    """An infinity among a layer's input activations (a BatchNorm bias of layer2's first block set to inf, as in
    test_gpu_parity.py) raises "infinity or a NaN" in adaptive mode as in every mode: nothing adapts to it."""
    sd = dict(synth.synthetic_state_dict(0))
    key = "_feature_extractor._image_backbone.0._layers.2.0.bn2.bias"
    sd[key] = sd[key].copy()
    sd[key][3] = np.float32(np.inf)
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16_always")
        eng.set_split_scale("adaptive")
        eng.split_adaptations(reset=True)
        eng.backbone(_dev(synth.synthetic_crops(8, seed=3)))
        with pytest.raises(FloatingPointError, match="infinity or a NaN"):
            eng.poll_status()
        eng.poll_status()
    finally:
        eng.close()


def test_modes_scopes_the_adaptive_split_scale(zero_bias):
    """modes(split_scale=...) scopes the mode: inside, an input 64 x the calibration set's computes and adapts; after the block
    the calibrated mode is back and the same input raises "range check" again; a mode already set is left alone."""
    sd, crops, _ref = zero_bias
    eng = _split_engine(sd, crops)
    try:
        bright = _dev(crops * np.float32(64.0))
        with eng.modes(split_scale="adaptive"):
            assert eng.split_scale == "adaptive"
            eng.split_adaptations(reset=True)
            eng.backbone(bright)
            eng.poll_status()
            assert eng.split_adaptations() > 0
        assert eng.split_scale == "calibrated"
        eng.backbone(bright)
        with pytest.raises(FloatingPointError, match="range check"):
            eng.poll_status()
        eng.set_split_scale("dynamic")
        with eng.modes(split_scale="adaptive"):
            pass
        assert eng.split_scale == "dynamic"
        assert math.isfinite(eng.backbone(bright).abs().max().item())
        eng.poll_status()
    finally:
        eng.close()
