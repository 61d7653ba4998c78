"""Shared by the per-stage tests of the backbone (test_stage_host.py, test_gpu_backbone_stages.py): routing networks that
carry the output of ONE stage - the stem or one of the 12 BasicBlocks - unchanged to the final [N,72,6,6] feature map, the
bookkeeping of which stage element each final element shows, and the per-element magnitude rounding errors are held to.

A routing network keeps the given weights up to and including the stage.  Every later block without a shortcut convolution
computes relu(x + 0) = x (conv1 = conv2 = 0), every later block with one (layers.2.0, 3.0, 4.0) copies input pixel
(2i + oy, 2j + ox) of input channel c to output pixel (i, j) of output channel g cin + c - one offset per group g in {0, 1} -
and the projection picks 72 consecutive channels.  All router arithmetic is x 1 and + 0."""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from absolutetrack_amd import arch
from oracle import ref_model

_BB = "_feature_extractor._image_backbone"
_BLOCKS = arch.backbone_blocks()
STAGES = ["stem"] + [p[len(_BB) + 3:] for p, *_ in _BLOCKS]       # the keys ref_model.backbone's taps use, "proj" left out
# folded to exactly 1.0f by ut_weights.cpp (g / sqrt(var + 1e-5) in double): var + 1e-5 is within 3e-8 of 1
ROUTER_VAR = np.float32(1 - 1e-5)


def stage_geometry(stage: str) -> Tuple[int, int, List[int]]:
    """(channels, height = width, indices into arch.backbone_blocks() of the shortcut-convolution blocks AFTER the stage)."""
    if stage == "stem":
        bi, ch, hw = -1, arch.STEM_PLANES, arch.CROP // 2
    else:
        bi = STAGES.index(stage) - 1
        ch = _BLOCKS[bi][2]
        hw = arch.CROP // 2
        for _p, _ci, _co, s, _ds in _BLOCKS[: bi + 1]:
            hw //= s
    return ch, hw, [b for b in range(bi + 1, len(_BLOCKS)) if _BLOCKS[b][4]]


def _router_bn(sd, p, c):
    sd[p + ".weight"] = np.ones(c, np.float32)
    sd[p + ".bias"] = np.zeros(c, np.float32)
    sd[p + ".running_mean"] = np.zeros(c, np.float32)
    sd[p + ".running_var"] = np.full(c, ROUTER_VAR, np.float32)


def router_keys(stage: str) -> List[str]:
    """Prefixes of the blocks a routing network for `stage` replaces."""
    first = 0 if stage == "stem" else STAGES.index(stage)
    return [p for p, *_ in _BLOCKS[first:]]


def router_state_dict(sd: Dict[str, np.ndarray], stage: str, offsets, chan0: int):
    """(state dict, selection).  offsets: for each shortcut-convolution block after the stage, in network order, the two
    (oy, ox) pixel offsets of its output groups 0 and 1; chan0: first of the 72 layer4 channels the projection picks.
    selection[k] = (c, oy, ox, mult): final element (k, i, j) is stage element (c, mult i + oy, mult j + ox) (None: the final
    channel shows nothing)."""
    _ch, _hw, routers = stage_geometry(stage)
    assert len(offsets) == len(routers) and 0 <= chan0 <= arch.LAYER_PLANES[-1] - arch.FEAT_CH
    out = dict(sd)
    first = 0 if stage == "stem" else STAGES.index(stage)
    for bi in range(first, len(_BLOCKS)):
        p, cin, cout, _stride, ds = _BLOCKS[bi]
        w1 = np.zeros((cout, cin, 3, 3), np.float32)
        w2 = np.zeros((cout, cout, 3, 3), np.float32)
        if ds:
            assert cout == 2 * cin
            for g, (oy, ox) in enumerate(offsets[routers.index(bi)]):
                assert oy in (0, 1) and ox in (0, 1)
                w1[g * cin + np.arange(cin), np.arange(cin), 1 + oy, 1 + ox] = 1.0
            w2[np.arange(cout), np.arange(cout), 1, 1] = 1.0
            out[p + ".downsample.0.weight"] = np.zeros((cout, cin, 1, 1), np.float32)
            _router_bn(out, p + ".downsample.1", cout)
        out[p + ".conv1.weight"], out[p + ".conv2.weight"] = w1, w2
        _router_bn(out, p + ".bn1", cout)
        _router_bn(out, p + ".bn2", cout)
    wp = np.zeros((arch.FEAT_CH, arch.LAYER_PLANES[-1], 1, 1), np.float32)
    wp[np.arange(arch.FEAT_CH), chan0 + np.arange(arch.FEAT_CH)] = 1.0
    out[f"{_BB}.1.weight"] = wp
    out[f"{_BB}.1.bias"] = np.zeros(arch.FEAT_CH, np.float32)
    selection = []
    for k in range(arch.FEAT_CH):
        c, oy, ox = chan0 + k, 0, 0
        for s in range(len(routers) - 1, -1, -1):       # walk back from layer4 to the stage
            cin = _BLOCKS[routers[s]][1]
            g, c = divmod(c, cin)
            oy += offsets[s][g][0] << s
            ox += offsets[s][g][1] << s
        selection.append((c, oy, ox, 1 << len(routers)))
    return out, selection


def gather(tap: torch.Tensor, selection) -> torch.Tensor:
    """[N,72,6,6] in tap's dtype: the elements of the stage's map [N,C,H,W] that `selection` shows."""
    out = torch.zeros(tap.shape[0], arch.FEAT_CH, arch.FEAT_HW, arch.FEAT_HW, dtype=tap.dtype)
    for k, sel in enumerate(selection):
        if sel is not None:
            c, oy, ox, mult = sel
            out[:, k] = tap[:, c, oy::mult, ox::mult]
    return out


def _bits(v: int, n: int) -> List[int]:
    return [(v >> s) & 1 for s in range(n)]


def _handle(n_routers: int, chan0: int, by_group: Dict[Tuple[int, ...], Tuple[int, int]]):
    """offsets that give group path (g of router 0, g of router 1, ..) the composite offset by_group[path]; paths that share a
    group at some router must agree on that router's bit."""
    offsets: List[List[Optional[Tuple[int, int]]]] = [[None, None] for _ in range(n_routers)]
    for path, (oy, ox) in by_group.items():
        for s, g in enumerate(path):
            bit = (_bits(oy, n_routers)[s], _bits(ox, n_routers)[s])
            assert offsets[s][g] in (None, bit)
            offsets[s][g] = bit
    return tuple(tuple(o if o is not None else (0, 0) for o in pair) for pair in offsets), chan0


def router_plan(stage: str):
    """[(offsets, chan0)]: the handles of a stage, 8 at the most.  Over the plan every row and every column of the stage's map,
    its four corner pixels and every channel are observed (test_stage_host.py asserts that from the selection maps).
      32 channels (48 x 48, three routers, mult 8): layer4 channels 96..127 come through groups (1, 1, 0) of the three routers and
        128..159 through (0, 0, 1) - no router group in common, so chan0 = 96 shows all 32 channels at two independent offsets:
        both diagonals, (r, r) and (r, 7 - r), r = 0..7, in eight handles;
      64 channels (24 x 24, mult 4): chan0 = 64 shows all 64 channels through groups (1, 0) and channels 0..7 through (0, 1): both
        diagonals on the first, the offsets two columns further on the second, eight handles;
      128 channels (12 x 12, mult 2): the windows 0 and 56 (group 0) at offsets (0, 0), (1, 1) and the windows 128 and 184
        (group 1) at (0, 1), (1, 0): every channel at every offset - the whole map - in eight handles;
      256 channels (6 x 6): the windows 0, 72, 144, 184 - the whole map."""
    ch, _hw, routers = stage_geometry(stage)
    n = len(routers)
    if ch == 32:
        pairs = [((r, r), (7 - r, 7 - r)) for r in range(4)] + [((r, 7 - r), (7 - r, r)) for r in range(4)]
        return [_handle(n, 96, {(1, 1, 0): a, (0, 0, 1): b}) for a, b in pairs]
    if ch == 64:
        first = [(r, r) for r in range(4)] + [(r, 3 - r) for r in range(4)]
        return [_handle(n, 64, {(1, 0): (oy, ox), (0, 1): (oy, (ox + 2) % 4)}) for oy, ox in first]
    if ch == 128:
        return ([_handle(n, c0, {(0,): o}) for c0 in (0, 56) for o in ((0, 0), (1, 1))] +
                [_handle(n, c0, {(1,): o}) for c0 in (128, 184) for o in ((0, 1), (1, 0))])
    return [((), c0) for c0 in (0, 72, 144, 184)]


def coverage(stage: str, selections):
    """(rows, columns, channels, pixels (y, x) of channel-independent interest) observed by a list of selection maps."""
    rows, cols, chans, pixels = set(), set(), set(), set()
    for selection in selections:
        for sel in selection:
            if sel is None:
                continue
            c, oy, ox, mult = sel
            chans.add(c)
            ys = [mult * i + oy for i in range(arch.FEAT_HW)]
            xs = [mult * j + ox for j in range(arch.FEAT_HW)]
            rows.update(ys)
            cols.update(xs)
            pixels.update((y, x) for y in ys for x in xs)
    return rows, cols, chans, pixels


# ---------------------------------------------------------------- the scale of an element's rounding error
def _folded(sd64, conv, bn, bias=None):
    """(w', b') in float64: eval-mode BatchNorm folded into the convolution."""
    w = sd64[conv]
    b = sd64[bias] if bias is not None else torch.zeros(w.shape[0], dtype=w.dtype)
    if bn is None:
        return w, b
    s = sd64[bn + ".weight"] / torch.sqrt(sd64[bn + ".running_var"] + arch.BN_EPS)
    return w * s[:, None, None, None], (b - sd64[bn + ".running_mean"]) * s + sd64[bn + ".bias"]


def _abs_conv(x, wb, stride, pad):
    return F.conv2d(x, wb[0].abs(), wb[1].abs(), stride, pad)


def magnitude(sd64, stage: str, x_in: torch.Tensor) -> torch.Tensor:
    """a[e]: the stage evaluated in float64 with the absolute values of its folded weights and shifts on |input| (x_in: the
    crops [N,96,96] for the stem, else the previous stage's map).  It bounds every partial sum of element e, in any order of
    summation, so an fp32 chain's rounding error in e is proportional to it.  `stage` may be "proj"."""
    x = x_in.double().abs()
    if stage == "stem":
        p = f"{_BB}.0._layers.0"
        return F.max_pool2d(_abs_conv(x.unsqueeze(1), _folded(sd64, p + ".0.weight", p + ".1", p + ".0.bias"), 1, 1), 2, 2)
    if stage == "proj":
        return _abs_conv(x, _folded(sd64, f"{_BB}.1.weight", None, f"{_BB}.1.bias"), 1, 0)
    p, _cin, _cout, stride, ds = _BLOCKS[STAGES.index(stage) - 1]
    h = _abs_conv(x, _folded(sd64, p + ".conv1.weight", p + ".bn1"), stride, 1)
    h = _abs_conv(h, _folded(sd64, p + ".conv2.weight", p + ".bn2"), 1, 1)
    if ds:
        return h + _abs_conv(x, _folded(sd64, p + ".downsample.0.weight", p + ".downsample.1"), stride, 0)
    return h + x


def stage_input(stage: str, crops: torch.Tensor, taps: dict) -> torch.Tensor:
    """The tensor `stage` reads, from the taps of ref_model.backbone on `crops`."""
    if stage == "stem":
        return crops
    if stage == "proj":
        return taps[STAGES[-1]]
    return taps[STAGES[STAGES.index(stage) - 1]]


# ---------------------------------------------------------------- inputs
def _edge_crops() -> np.ndarray:
    c = arch.CROP
    e = np.zeros((3, c, c), np.float32)
    e[0] = 1.0
    for y, x in ((0, 0), (0, c - 1), (c - 1, 0), (c - 1, c - 1), (47, 48)):
        e[1, y, x] = 1.0
    yy, xx = np.mgrid[0:c, 0:c]
    e[2] = ((yy + xx) % 2).astype(np.float32)
    return e


EDGE_CROPS = _edge_crops()      # constant 1 | single 1.0 pixels at the corners and at (47, 48) | 0/1 checkerboard
N_SYNTH = 3


def stage_crops() -> np.ndarray:
    """The 6 crops of the stage tests: synthetic_crops(3, seed=3), then EDGE_CROPS."""
    from absolutetrack_amd import synth
    return np.concatenate([synth.synthetic_crops(N_SYNTH, seed=3), EDGE_CROPS])


def sd64(sd):
    return {k: v.double() for k, v in ref_model.to_torch_state_dict(sd).items()}


def references(sd):
    """(crops [6,96,96] float32, taps of the float64 oracle, taps of the fp32 oracle, {stage or "proj": a}, {..: r32}) of the
    network `sd` on stage_crops(): r32 = max_e |tap32 - tap64| / a over the elements with a > 0."""
    crops = stage_crops()
    s64, s32 = sd64(sd), ref_model.to_torch_state_dict(sd)
    t64, t32 = {}, {}
    with torch.no_grad():
        ref_model.backbone(s64, torch.from_numpy(crops).double(), t64)
        ref_model.backbone(s32, torch.from_numpy(crops), t32)
        a, r32 = {}, {}
        for stage in STAGES + ["proj"]:
            a[stage] = magnitude(s64, stage, stage_input(stage, torch.from_numpy(crops).double(), t64))
            err = (t32[stage].double() - t64[stage]).abs()
            assert bool((err[a[stage] == 0] == 0).all())
            r32[stage] = (err / a[stage].clamp_min(1e-300)).max().item()
    return crops, t64, t32, a, r32
