"""CPU tests: the float64 oracle and the test networks the split-fp16 range tests (test_gpu_split_range.py) are built on.
oracle/ref_model.py follows the dtype of its inputs; a float64 state dict is `to_torch_state_dict` plus `.double()`."""
import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, synth
from oracle import ref_model, scenarios


def _sd64(sd):
    return {k: v.double() for k, v in ref_model.to_torch_state_dict(sd).items()}


@pytest.mark.parametrize("known", [True, False])
def test_fp64_oracle_agrees_with_fp32_oracle_on_golden_scenarios(known):
    """The two golden scenarios (two steps on the same slots, the second with warm memory) through the oracle in fp32 and in
    fp64: every output is float64 in the second run - no stage falls back to a float32 constant - and the two agree at fp32
    rounding (measured: at most 4.8e-7 of an output's largest magnitude - the wrist transforms - and 9.0e-7 of the memory's)."""
    sd = synth.synthetic_state_dict(0)
    m32 = ref_model.OracleModel(sd)
    m64 = ref_model.OracleModel(sd)
    m64.sd = _sd64(sd)
    axes, rest = (torch.from_numpy(a) for a in scenarios.skeleton_m())
    for st in scenarios.model_steps(known):
        t = {k: torch.from_numpy(v) for k, v in st.items()}
        t64 = {k: v.double() if v.is_floating_point() else v for k, v in t.items()}
        o32 = m32.forward(t["images"], t["intrinsics"], t["extrinsics"], t["sample_range"], t["memory_idx"], t["use_memory"],
                          t["hand_idx"], axes, rest, known_skeleton=known)
        o64 = m64.forward(t64["images"], t64["intrinsics"], t64["extrinsics"], t64["sample_range"], t64["memory_idx"],
                          t64["use_memory"], t64["hand_idx"], axes.double(), rest.double(), known_skeleton=known)
        for k in ("raw", "joint_angles", "wrist_xfs", "landmark_uncertainty_sigmas") + (() if known else ("skel_scales",)):
            assert o64[k].dtype == torch.float64, k
            scale = o64[k].abs().max().item()
            assert (o32[k].double() - o64[k]).abs().max().item() < 2e-6 * scale, k
        assert m64.temporal.mem.dtype == torch.float64 and m64.temporal.prev_ext.dtype == torch.float64
        scale = m64.temporal.mem.abs().max().item()
        assert (m32.temporal.mem.double() - m64.temporal.mem).abs().max().item() < 2e-6 * scale


def test_zero_bias_backbone_is_positively_homogeneous_in_fp64():
    """zero_bias_state_dict: backbone(c x 2^j) == 2^j x backbone(c), bit for bit in fp64 (power-of-two scaling commutes with
    every rounding of a network without additive terms) - the identity that gives test_gpu_split_range.py its reference at
    every scale from one fp64 run.  The additive terms are what breaks it: the plain network is not homogeneous."""
    sd = synth.synthetic_state_dict(0)
    z = _sd64(synth.zero_bias_state_dict(sd))
    crops = torch.from_numpy(synth.synthetic_crops(2, seed=21)).double()
    ref = ref_model.backbone(z, crops)
    assert ref.abs().max().item() > 0
    for j in (-24, -12, 0, 5):
        assert torch.equal(ref_model.backbone(z, crops * 2.0 ** j), ref * 2.0 ** j), j
    plain = _sd64(sd)
    assert not torch.allclose(ref_model.backbone(plain, crops * 32.0), 32.0 * ref_model.backbone(plain, crops), rtol=1e-3)


def _canonical_layer1(sd):
    flat = _native.canonical_backbone_weights(sd)
    pos = 0

    def take(cout, cin, k):
        nonlocal pos
        w = flat[pos: pos + cout * cin * k * k].reshape(cout, cin * k * k)
        pos += w.size
        b = flat[pos: pos + cout]
        pos += cout
        return w.astype(np.float64), b.astype(np.float64)
    stem = take(32, 1, 3)
    return stem, [(take(32, 32, 3), take(32, 32, 3)) for _ in range(2)]


def test_layer1_worst_case_network_survives_canonical_packing():
    """layer1_worst_case_state_dict as ut_create packs it (ut_canonical_backbone_weights, host only): the stem's rows are one
    all-positive row and its bias 0, so a constant crop gives the stem output's maximum on every channel; in both layer1 blocks
    every conv1 row is one all-positive row with no bias - each intermediate channel reaches the L1 bound max|x| x
    max_c sum_k |w1[c][k]| that conv_block32.hip scales by, at the top of its octave - and bn2(conv2(.)) returns its input."""
    sd = synth.layer1_worst_case_state_dict(synth.synthetic_state_dict(0))
    (sw, sb), blocks = _canonical_layer1(sd)
    assert (sw > 0).all() and (sw == sw[:1]).all() and (sb == 0).all()
    for (w1, b1), (w2, b2) in blocks:
        assert (w1 > 0).all() and (w1 == w1[:1]).all() and (b1 == 0).all()
        l1 = np.abs(w1).sum(1)
        assert l1.max() == w1[0].sum()
        sig = l1.max() / 2.0 ** np.floor(np.log2(l1.max()))
        assert 1.9 < sig < 2.0, sig
        assert (w2 > 0).all() and (b2 == 0).all()
        assert abs(w1[0].sum() * w2[0].sum() - 1.0) < 1e-6
