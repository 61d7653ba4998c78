"""GPU tests of conv_w4.hip's chains: the consecutive stride-1 3x3 convolutions of layer2, layer3, layer4 and of the regressor as
one launch each (ut_set_resident_weights kinds 1 .. 6) against one launch per convolution (kind 7).

Per layer a chain computes the same products in the same order on the same tensors, so every comparison here is torch.equal:
no tolerance is involved.  What differs is who runs a tile when, which is what the crop counts walk through: a workgroup with a
single unit (every item starts behind its producer's epilogue), two units in flight, refills from the ticket queue, ragged last
tiles, and the two-column units of layer4."""
import math

import numpy as np
import pytest
import torch

from absolutetrack_amd import _native

from test_gpu_parity import DEV, _dev, _head_call, _head_inputs, split_engine  # noqa: F401  (split_engine: the fixture)
from test_gpu_split_range import _guard, _raises, zero_bias  # noqa: F401  (zero_bias: the fixture)
from absolutetrack_amd import synth

pytestmark = pytest.mark.gpu

CHAINED, PER_LAYER = 1, 7


def _with_kind(eng, kind, fn):
    eng.set_resident_weights(kind)
    try:
        return fn()
    finally:
        eng.set_resident_weights(1)


# 1: half a 12x12 tile, an eighth of a 6x6 tile - one workgroup, one unit.  2: one exact 12x12 tile.  5, 37: ragged last tiles.
# 300: 300 units on 256 workgroups at 24x24 (two in flight, one alone), one unit per workgroup at 12x12.  600: the same at 12x12.
# 1100: 550 units at 12x12 (two in flight and a refill), 1100 at 24x24 (several refills).
# Layer4's two-column units chain only from as many units as the chip has CUs (conv_w4_chain_fills: 2048 crops on 256 CUs; below
# that its convolutions keep their own launches, in both kinds).  2060: 258 two-column units, the last one ragged - two in flight
# on the first workgroups, one alone (restarting at every other item) on the rest; 12x12 and 24x24 in several rounds.
@pytest.mark.parametrize("n_crops", [1, 2, 5, 37, 300, 600, 1100, 2060])
def test_chained_backbone_equals_one_launch_per_convolution(split_engine, n_crops):
    base = synth.synthetic_crops(min(n_crops, 37), seed=11)
    crops = _dev(base)
    if n_crops > 37:      # (the 37 crops over and over, each copy at its own gain: no two tiles alike)
        reps = (n_crops + 36) // 37
        crops = crops.repeat(reps, 1, 1)[:n_crops] * torch.linspace(0.5, 1.5, n_crops, device=DEV)[:, None, None]
    want = _with_kind(split_engine, PER_LAYER, lambda: split_engine.backbone(crops).clone())
    got = _with_kind(split_engine, CHAINED, lambda: split_engine.backbone(crops).clone())
    again = _with_kind(split_engine, CHAINED, lambda: split_engine.backbone(crops).clone())
    split_engine.poll_status()
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(again, got)


# S samples of the regressor's 6x6 maps, eight to a tile: 1 and 8 - one (partial, exact) tile; 9 - a ragged second tile; 300 - 38
# workgroups of one unit each, the case where no item has another unit's item to hide its start behind
@pytest.mark.parametrize("n_samples", [1, 8, 9, 300])
def test_chained_regressor_equals_one_launch_per_convolution(split_engine, n_samples):
    d = _head_inputs(split_engine, n_samples=n_samples, seed=5)

    def head():
        split_engine.reset_memory()
        return _head_call(split_engine, d)

    want = _with_kind(split_engine, PER_LAYER, head)
    got = _with_kind(split_engine, CHAINED, head)
    again = _with_kind(split_engine, CHAINED, head)
    split_engine.poll_status()
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(again, got)


def test_chain_guard_raises_where_the_launches_do(zero_bias):
    """Zero-bias network, calibrated on its 16 crops: backbone(f C) scales every tensor by f, and tensor t leaves its calibrated
    range at f = _guard(word_t).  The tensors a chain's second and later layers read (block outputs and inner tensors of layer2's
    b2 .. b4 and layer3's b5 .. b9: ids 6 .. 9, 12 .. 19) are guarded inside the chain, item by item (layer4's, ids 22 .. 23, by
    their own launches at this batch size); just above each of their guards - and at 64, where the stem's output trips the first
    launch - kind 1 and kind 7 raise "range check" at the same calls, and below the smallest guard neither does and the features
    are equal."""
    sd, crops, ref = zero_bias
    eng = _native.HipEngine(sd, DEV)
    try:
        eng.set_conv_arithmetic("split_f16_always")
        eng.calibrate_split(_dev(crops))
        words = eng.split_calibration()
        inner = [6, 7, 8, 9] + list(range(12, 20)) + [22, 23]
        guards = sorted({_guard(words[t]) for t in inner if words[t] > 0})
        assert guards and all(32.0 < g <= 64.0 for g in guards)
        others = min(_guard(words[t]) for t in range(24) if t not in inner and words[t] > 0)
        print(f"\nguards of the tensors inside chains {[round(g, 3) for g in guards]}, smallest other guard {others:.3f}")
        f_safe = math.floor(min(_guard(w) for w in words[:24] if w > 0) * 0.999 * 8) / 8
        fs = [1.0, 16.0, f_safe] + [g * 1.01 for g in guards] + [64.0]
        res = {}
        for kind in (CHAINED, PER_LAYER):
            eng.set_resident_weights(kind)
            res[kind] = []
            for f in fs:      # (test_gpu_split_range._sweep's loop, keeping the features)
                got = eng.backbone(_dev(crops * np.float32(f))).clone()
                res[kind].append((f, _raises(eng), got))
        for (f, r1, o1), (_f, r7, o7) in zip(res[CHAINED], res[PER_LAYER]):
            assert r1 == r7, f
            if not r1:
                assert torch.equal(o1, o7), f
        raised = {f: r for f, r, _o in res[CHAINED]}
        assert not raised[1.0] and not raised[16.0] and not raised[f_safe]
        assert all(raised[g * 1.01] for g in guards) and raised[64.0]
    finally:
        eng.close()


@pytest.mark.parametrize("setup", ["dynamic", "adaptive", "no_fusion"])
def test_modes_without_chains_keep_their_launches(setup):
    """Dynamic and adaptive scale modes and ut_set_block_fusion(0) launch every convolution by itself under every kind: kind 1
    gives kind 7's features there."""
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        if setup == "dynamic":
            eng.set_split_scale("dynamic")
        eng.set_conv_arithmetic("split_f16_always")
        if setup == "adaptive":
            eng.set_split_scale("adaptive")
        if setup == "no_fusion":
            eng.set_block_fusion(False)
        crops = _dev(synth.synthetic_crops(37, seed=13))
        want = _with_kind(eng, PER_LAYER, lambda: eng.backbone(crops).clone())
        got = _with_kind(eng, CHAINED, lambda: eng.backbone(crops).clone())
        eng.poll_status()
        assert torch.isfinite(want).all()
        assert torch.equal(got, want)
    finally:
        eng.close()
