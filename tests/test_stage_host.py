"""CPU tests of the routing networks (stage_cases.py) that test_gpu_backbone_stages.py observes single backbone stages through:
in float64 a routing network's output IS the selected elements of the stage's map, its plan reaches every row, column, corner
and channel, ut_create's host packing turns every router operation into an exact one, the references are not mostly zeros, and
the per-element magnitude a[e] is a scale an fp32 chain's rounding follows.  Measured figures are in the docstrings."""
import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, arch, synth
from oracle import ref_model

import stage_cases as sc


@pytest.fixture(scope="module")
def net():
    sd = synth.synthetic_state_dict(0)
    return (sd,) + sc.references(sd)


def _canonical(sd):
    """ut_canonical_backbone_weights as {"stem" | block prefix + ".conv1" / ".conv2" / ".ds" | "proj": (w [cout,cin,taps], b)}."""
    flat = _native.canonical_backbone_weights(sd)
    pos = 0

    def take(cout, cin, taps):
        nonlocal pos
        w = flat[pos: pos + cout * cin * taps].reshape(cout, cin, taps)
        pos += w.size
        b = flat[pos: pos + cout]
        pos += cout
        return w, b
    out = {"stem": take(arch.STEM_PLANES, 1, 9)}
    for p, cin, cout, _s, ds in arch.backbone_blocks():
        out[p + ".conv1"] = take(cout, cin, 9)
        out[p + ".conv2"] = take(cout, cout, 9)
        if ds:
            out[p + ".ds"] = take(cout, cin, 1)
    out["proj"] = take(arch.FEAT_CH, arch.LAYER_PLANES[-1], 1)
    assert pos == flat.size
    return out


@pytest.mark.parametrize("stage", sc.STAGES)
def test_router_network_shows_the_stage_in_fp64(net, stage):
    """For every handle of the stage's plan, the float64 oracle on the routing network against gather(tap of the natural
    network): within 1e-7 of the stage's largest magnitude (measured: at most 4.07e-8 - torch's BatchNorm applying
    1 / sqrt(float32(1 - 1e-5) + 1e-5) once per router - and exactly 0 for layer4's stages), and at least 1/3 of the reference
    elements of every crop are non-zero (measured: 0.417 or more, the smallest at the stem and at layers.3.0)."""
    sd, crops, t64, _t32, _a, _r32 = net
    x = torch.from_numpy(crops).double()
    scale = t64[stage].abs().max().item()
    worst, share = 0.0, 1.0
    for offsets, chan0 in sc.router_plan(stage):
        rsd, sel = sc.router_state_dict(sd, stage, offsets, chan0)
        with torch.no_grad():
            got = ref_model.backbone(sc.sd64(rsd), x)
        want = sc.gather(t64[stage], sel)
        worst = max(worst, (got - want).abs().max().item() / scale)
        share = min(share, (want != 0).reshape(len(crops), -1).double().mean(1).min().item())
    print(f"\n{stage}: router vs gather {worst:.3g} of the stage's largest, smallest non-zero share {share:.3f}")
    assert worst < 1e-7
    assert share >= 1 / 3


@pytest.mark.parametrize("stage", sc.STAGES)
def test_router_plan_covers_the_stage(stage):
    """Over a stage's plan (at most 8 handles) the selection maps reach every row, every column, the four corner pixels and
    every channel of the stage's map, and stay inside it."""
    ch, hw, routers = sc.stage_geometry(stage)
    plan = sc.router_plan(stage)
    assert 1 <= len(plan) <= 8
    sd = {}     # the selection does not depend on the weights
    sels = [sc.router_state_dict(sd, stage, offsets, chan0)[1] for offsets, chan0 in plan]
    for sel in sels:
        assert len(sel) == arch.FEAT_CH
        for c, oy, ox, mult in (s for s in sel if s is not None):
            assert mult == 2 ** len(routers) and mult * arch.FEAT_HW == hw
            assert 0 <= c < ch and 0 <= oy < mult and 0 <= ox < mult
    rows, cols, chans, pixels = sc.coverage(stage, sels)
    assert rows == set(range(hw)) and cols == set(range(hw)) and chans == set(range(ch))
    assert {(0, 0), (0, hw - 1), (hw - 1, 0), (hw - 1, hw - 1)} <= pixels


@pytest.mark.parametrize("stage", sc.STAGES)
def test_router_layers_pack_to_exact_copies(net, stage):
    """ut_canonical_backbone_weights of every routing network (host only): every folded weight of a router block is exactly
    0.0f or 1.0f and every router bias exactly 0 - each router tap exactly once per output channel - and the layers up to the
    stage pack to the natural network's bits.  The projection's weights are 0 or ONE power of two per row: ut_create keeps
    trunk channel c of the stage at a canonical scale 2^k_c (stored value = the checkpoint's value x 2^k_c, through every router
    after it), and the projection column that reads it carries 2^-k_c.  Asserted: that weight times the stage's 2^k_c, read off
    the stage's own packed shift, is exactly 1 - so in fp32 the routed output is the stage's value bit for bit."""
    sd, *_ = net
    natural = _canonical(sd)
    # 2^k_c of the stage's output channels: the packed shift of the convolution that writes them over the plainly folded one
    p = f"{sc._BB}.0._layers.0" if stage == "stem" else sc._BLOCKS[sc.STAGES.index(stage) - 1][0]
    s64 = sc.sd64(sd)
    _w, shift = (sc._folded(s64, p + ".0.weight", p + ".1", p + ".0.bias") if stage == "stem"
                 else sc._folded(s64, p + ".conv2.weight", p + ".bn2"))
    packed = natural["stem" if stage == "stem" else p + ".conv2"][1].astype(np.float64)
    ratio = packed / shift.numpy()
    k_c = np.round(np.log2(ratio))
    assert np.abs(ratio / 2.0 ** k_c - 1).max() < 1e-6
    router_blocks = sc.router_keys(stage)
    for offsets, chan0 in sc.router_plan(stage):
        rsd, sel = sc.router_state_dict(sd, stage, offsets, chan0)
        canon = _canonical(rsd)
        for name, (w, b) in canon.items():
            if name == "proj":
                assert (b == 0).all()
                for k, (c, _oy, _ox, _m) in enumerate(sel):
                    assert np.count_nonzero(w[k]) == 1
                    assert float(w[k, chan0 + k, 0]) * 2.0 ** k_c[c] == 1.0, (k, c)
            elif any(name.startswith(rp + ".") for rp in router_blocks):
                assert ((w == 0) | (w == 1)).all() and (b == 0).all(), name
                ones = np.count_nonzero(w.reshape(w.shape[0], -1), axis=1)
                has_ds = name[: name.rindex(".")] + ".ds" in canon
                assert (ones == (1 if has_ds and not name.endswith(".ds") else 0)).all(), name
            else:
                assert np.array_equal(w, natural[name][0]) and np.array_equal(b, natural[name][1]), name


def test_fp32_oracle_rounds_in_proportion_to_the_magnitude(net):
    """r32[stage] = max_e |tap32[e] - tap64[e]| / a[e] on the 6 crops, the oracle in fp32 torch against itself in float64, for
    the 13 stages and the projection: below 1e-6 everywhere, so a[e] (stage_cases.magnitude) is a usable per-element scale and
    4 x r32 a bound a GPU chain with the same unit roundoff can be held to.  a[e] > 0 for every element.  Measured: stem 2.24e-7;
    layers.1.0 2.58e-8, 1.1 4.25e-8; 2.0 5.40e-8, 2.1 4.05e-8, 2.2 4.08e-8; 3.0 3.71e-8, 3.1 2.39e-8, 3.2 2.36e-8, 3.3 2.95e-8,
    3.4 2.25e-8; 4.0 2.20e-8, 4.1 2.88e-8; projection 2.88e-7."""
    _sd, _crops, t64, _t32, a, r32 = net
    print("\nr32:", " ".join(f"{s}:{r32[s]:.3g}" for s in sc.STAGES + ["proj"]))
    for stage in sc.STAGES + ["proj"]:
        assert a[stage].shape == t64[stage].shape
        assert bool((a[stage] * (1 + 1e-12) >= t64[stage].abs()).all())       # it bounds the value itself
        assert 0 < r32[stage] < 1e-6, stage


# (stage, which convolution, (cout, cin, ky, kx)): one tap of one weight whose input channel is alive on the 6 crops (a tap that
# reads a channel ReLU keeps at zero changes nothing anywhere)
_TAPS = [("_layers.1.0", "conv1", (5, 7, 0, 2)), ("_layers.2.0", "downsample.0", (40, 9, 0, 0)),
         ("_layers.3.2", "conv2", (127, 64, 2, 2)), ("_layers.4.1", "conv2", (200, 31, 1, 0))]


@pytest.mark.parametrize("stage,conv,tap", _TAPS, ids=[f"{s}.{c}" for s, c, _t in _TAPS])
def test_stage_bound_sees_one_perturbed_tap(net, stage, conv, tap):
    """What the per-stage bound buys, on the oracle alone: the fp32 oracle with ONE tap of one weight of a stage zeroed, and
    with that tap 2^-8 too small (a lost second fp16 piece), against the float64 taps of the intact network.  R_stage: the
    error at the stage that owns the tap, over the elements its plan observes, in units of the allowance 4 r32 a[e]; R_out: the
    error at the final feature map in units of test_backbone_matches_oracle's 2e-5 x max(1, scale).  Asserted: the zeroed tap
    fails its stage by R_stage > 50, the 2^-8 tap by R_stage > 1, and both R_stage > 5 R_out.  Measured (R_stage / R_out), zeroed
    and 2^-8: layers.1.0 conv1 8.9e3 / 26 and 35 / 0.10; layers.2.0 shortcut 1.5e4 / 412 and 59 / 1.6; layers.3.2 conv2
    3.4e3 / 20 and 13 / 0.085; layers.4.1 conv2 3.3e3 / 55 and 13 / 0.21 - three of the four 2^-8 taps pass at the output.  The
    plan observes every channel at a subset of its pixels, so a defect confined to unobserved pixels of one channel is the limit
    of the method."""
    sd, crops, t64, _t32, a, r32 = net
    key = f"{sc._BB}.0.{stage}.{conv}.weight"
    assert sd[key][tap] != 0
    observed = torch.zeros_like(a[stage], dtype=torch.bool)
    for offsets, chan0 in sc.router_plan(stage):
        for c, oy, ox, mult in sc.router_state_dict({}, stage, offsets, chan0)[1]:
            observed[:, c, oy::mult, ox::mult] = True
    out_tol = 2e-5 * max(1.0, t64["proj"].abs().max().item())
    res = {}
    for factor in (0.0, 1 - 2.0 ** -8):
        broken = dict(sd)
        broken[key] = sd[key].copy()
        broken[key][tap] *= np.float32(factor)
        taps = {}
        with torch.no_grad():
            ref_model.backbone(ref_model.to_torch_state_dict(broken), torch.from_numpy(crops), taps)
        r_stage = ((taps[stage].double() - t64[stage]).abs() / (4 * r32[stage] * a[stage]))[observed].max().item()
        r_out = (taps["proj"].double() - t64["proj"]).abs().max().item() / out_tol
        res[factor] = (r_stage, r_out)
    print(f"\n{stage}.{conv}{tap}:", " ".join(f"x{f:g}: {rs:.3g} / {ro:.3g}" for f, (rs, ro) in res.items()))
    r_stage, r_out = res[0.0]
    assert r_stage > 50.0 and r_stage > 5.0 * r_out
    r_stage, r_out = res[1 - 2.0 ** -8]
    assert r_stage > 1.0 and r_stage > 5.0 * r_out
