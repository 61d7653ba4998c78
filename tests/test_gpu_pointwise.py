"""GPU tests of the streaming 1x1 convolutions (csrc/conv_pw.hip): the head's fusion and temporal chains as one launch each, the
projection and the stride-2 shortcut of layer4 as one streaming launch each (layer3's shortcut measured no faster there and stays
on conv_igemm: the switch leaves it alone).  They feed every matrix instruction the
operands of the conv_igemm launches they replace, in the same order, so every comparison here is torch.equal between
set_block_fusion(False) (every convolution its own conv_igemm launch) and set_block_fusion(True) on one handle."""
import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, synth

import test_gpu_head_edges as he

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 2, 5, 37]      # M = 36 S pixels: below one 32-pixel tile + a rest, no multiple of 32, tiles straddling samples


@pytest.fixture(scope="module")
def sd():
    return synth.synthetic_state_dict(0)


def _head_two_steps(eng, fusion, steps, known, skel):
    """Both steps of `steps` from a cleared temporal state: [(pose, raw, memory, prev_ext)] per step."""
    eng.set_block_fusion(fusion)
    eng.reset_memory()
    out = []
    for f, feat in steps:
        pose, raw = he.call(eng, feat, f, known, skel)
        mem, ext = (t.cpu() for t in eng.get_memory())
        out.append((pose, raw, mem, ext))
    return out


@pytest.mark.parametrize("known", [True, False])
@pytest.mark.parametrize("s", SIZES)
def test_head_chains_have_the_bits_of_the_separate_launches(sd, s, known):
    """Known-skeleton mode: one- and two-view samples mixed; unknown mode: two views each.  Two consecutive steps, the second on
    the first's memory.  Pose records, raw, memory and prev_ext after each step.
    The switch also selects ftl_in's store form (off: every lane stores its own pixel's values, the order before the LDS staging;
    on: staged through LDS), in both of its branches - cat144 of the two-view samples, fused of the one-view samples - so the
    comparison covers the staged kernel against the direct one: everything compared is a function of those two tensors."""
    rng = np.random.default_rng(900 + 2 * s + known)
    skel = he._skeleton()
    steps = []
    for step in range(2):
        f = he.frame(rng, he.mixed_views(s, known), max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
        if step:
            f["use"] = torch.ones(f["s"], dtype=torch.bool)
        steps.append((f, he.features(rng, f["n"])))
    eng = _native.HipEngine(sd, DEV)
    try:
        separate = _head_two_steps(eng, False, steps, known, skel)
        chained = _head_two_steps(eng, True, steps, known, skel)
        for step, (a, b) in enumerate(zip(separate, chained)):
            for name, x, y in zip(("pose", "raw", "memory", "prev_ext"), a, b):
                assert torch.isfinite(x).all(), (step, name)
                assert torch.equal(x, y), (step, name, (x - y).abs().max().item())
        assert separate[1][2].abs().max() > 0          # the second step did read a memory
    finally:
        eng.close()


@pytest.mark.parametrize("n", SIZES)
def test_fp32_backbone_features_have_the_bits_of_the_separate_launches(sd, n):
    """Exact-fp32 arithmetic, where the switch changes nothing but these launches: the projection's NCHW store and layer4's
    stride-2 shortcut (four passes over N) at M = 36 n."""
    crops = he._dev(synth.synthetic_crops(n, seed=70 + n))
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_block_fusion(False)
        separate = eng.backbone(crops).cpu()
        eng.set_block_fusion(True)
        streamed = eng.backbone(crops).cpu()
        eng.poll_status()
        assert torch.isfinite(separate).all() and separate.abs().max() > 0
        assert torch.equal(separate, streamed), (separate - streamed).abs().max().item()
    finally:
        eng.close()


def test_streaming_launches_replace_eight_convolution_launches_by_four(sd):
    """Launch counts of one head call and one fp32 backbone call with the switch on and off (profiled launches: the convolutions):
    2 chains for 6 launches in the head, launches one for one in the backbone."""
    rng = np.random.default_rng(950)
    skel = he._skeleton()
    f = he.frame(rng, [2] * 5, max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
    feat = he.features(rng, f["n"])
    crops = he._dev(synth.synthetic_crops(3, seed=75))
    eng = _native.HipEngine(sd, DEV)
    try:
        counts = {}
        for fusion in (False, True):
            eng.set_block_fusion(fusion)
            eng.profile_begin()
            he.call(eng, feat, f, True, skel)
            head = sum(k[1] for k in eng.profile_end_by_kind())
            eng.profile_begin()
            eng.backbone(crops)
            counts[fusion] = (head, sum(k[1] for k in eng.profile_end_by_kind()))
        assert counts[False][0] - counts[True][0] == 4, counts
        assert counts[False][1] == counts[True][1], counts
    finally:
        eng.close()


def test_split_regressor_zero_k_slice_skipped_equals_walked(sd):
    """Split-fp16 regressor (conv arithmetic split_f16, S = 1024 two-view samples: the size from which the split head is chosen at
    256 CUs): its tensors are padded from 76 to 128 channels, and with the switch on conv_w4 walks three 32-channel slices of K
    instead of four.  The fourth holds zeros in activations and weights: raw and the pose records equal those of the walked
    form (torch.equal: +0 == -0).  The test sees results only: it cannot tell which of the two forms a launch took, so it does not
    show that the slice IS skipped with the switch on (the kernel trace does: DESIGN.md 4h)."""
    s = 1024
    if s < 4 * torch.cuda.get_device_properties(0).multi_processor_count:
        s = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(970)
    skel = he._skeleton()
    f = he.frame(rng, [2] * s, max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16")
        feat = eng.backbone(he._dev(synth.synthetic_crops(f["n"], seed=52))).cpu()
        eng.poll_status()
        got = {}
        for fusion in (False, True):
            eng.set_block_fusion(fusion)
            eng.reset_memory()
            eng.profile_begin()
            got[fusion] = he.call(eng, feat, f, True, skel)
            assert eng.profile_end_by_kind()[1][1] == 4          # the regressor's four convolutions ran in the split arithmetic
        for name, x, y in zip(("pose", "raw"), got[False], got[True]):
            assert torch.isfinite(x).all() and x.abs().max() > 0, name
            assert torch.equal(x, y), (name, (x - y).abs().max().item())
    finally:
        eng.close()


def test_latency_mode_is_untouched_by_the_switch(sd):
    """Latency mode keeps its split-K call path whatever the switch says: backbone features and head outputs equal."""
    rng = np.random.default_rng(960)
    skel = he._skeleton()
    f = he.frame(rng, [2, 1], max_angle=1.2, max_t=0.3, focal=(100.0, 160.0))
    crops = he._dev(synth.synthetic_crops(f["n"], seed=80))
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_latency_mode(True)
        got = {}
        for fusion in (False, True):
            eng.set_block_fusion(fusion)
            eng.reset_memory()
            feat = eng.backbone(crops).cpu()
            pose, raw = he.call(eng, feat, f, True, skel)
            got[fusion] = (feat, pose, raw) + tuple(t.cpu() for t in eng.get_memory())
        for x, y in zip(got[False], got[True]):
            assert torch.equal(x, y)
    finally:
        eng.close()
