"""How far from float64 is ONE fp32 accumulation chain per output element?  (CPU study, TEST INFRASTRUCTURE ONLY.)

tests/test_gpu_backbone_stages.py holds each backbone stage to 4 x r32 a[e], r32 being the distance of the fp32 oracle (torch's
CPU convolution) from the float64 one in units of the element's magnitude bound a[e].  The exact-fp32 kernels (conv_igemm.hip,
conv_patch.hip) start an accumulator at bias + residual and add all K = 9 cin products to it one after another, k ordered
(32-channel slice, tap, channel); torch's convolution keeps several partial sums and rounds less.  This script runs the 12
BasicBlocks as that plain chain in numpy float32 (BatchNorm folded as ut_create folds it, each block fed the chain's own previous
output, the stem from the fp32 oracle) on the 6 crops of the stage tests and prints max |chain - fp64| / (r32 a[e]) per stage:
the figure a correct kernel of that structure shows, and the reason behind the entries of FP32_MARGIN_AT.  Takes about a minute.

    python -m oracle.studies.fp32_chain
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from absolutetrack_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import stage_cases as sc  # noqa: E402


def chain(x, w, b, stride, pad, res=None):
    """x [N,C,H,H] and folded w [co,ci,kh,kw], b [co] in float32 -> [N,co,Ho,Ho]: acc = b (+ res), then acc += w x, one k at a time."""
    n, _c, h, _ = x.shape
    co, ci, kh, kw = w.shape
    cols = F.unfold(torch.from_numpy(x), (kh, kw), padding=pad, stride=stride).numpy()
    p = cols.shape[2]
    cols = cols.reshape(n, ci, kh * kw, p)
    wk = w.reshape(co, ci, kh * kw)
    acc = np.broadcast_to(b[None, :, None], (n, co, p)).astype(np.float32).copy()
    if res is not None:
        acc = acc + res.reshape(n, co, p)
    for s0 in range(0, ci, 32):
        for t in range(kh * kw):
            for ch in range(s0, min(s0 + 32, ci)):
                acc = acc + wk[None, :, ch, t, None] * cols[:, None, ch, t, :]
    ho = (h + 2 * pad - kh) // stride + 1
    return acc.reshape(n, co, ho, ho)


def main():
    sd = synth.synthetic_state_dict(0)
    _crops, t64, t32, a, r32 = sc.references(sd)
    s64 = sc.sd64(sd)

    def f32(wb):
        return wb[0].numpy().astype(np.float32), wb[1].numpy().astype(np.float32)

    x = t32["stem"].numpy()
    for bi, (p, _cin, _cout, stride, ds) in enumerate(sc._BLOCKS):
        stage = sc.STAGES[bi + 1]
        w1, b1 = f32(sc._folded(s64, p + ".conv1.weight", p + ".bn1"))
        w2, b2 = f32(sc._folded(s64, p + ".conv2.weight", p + ".bn2"))
        h = np.maximum(chain(x, w1, b1, stride, 1), 0)
        res = chain(x, *f32(sc._folded(s64, p + ".downsample.0.weight", p + ".downsample.1")), stride, 0) if ds else x
        x = np.maximum(chain(h, w2, b2, 1, 1, res), 0)
        ratio = np.abs(x.astype(np.float64) - t64[stage].numpy()) / (r32[stage] * a[stage].numpy())
        print(f"{stage}: r32 {r32[stage]:.3g}, chain / (r32 a) all crops {ratio.max():.2f}, per crop",
              np.round(ratio.reshape(len(ratio), -1).max(1), 2), flush=True)


if __name__ == "__main__":
    main()
