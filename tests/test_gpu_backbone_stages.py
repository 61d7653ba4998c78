"""GPU tests of the backbone ONE STAGE AT A TIME against the float64 oracle, through ut_backbone alone: for the stem and each of
the 12 BasicBlocks, routing networks (stage_cases.py; test_stage_host.py checks them on the CPU) carry the stage's output
unchanged to the final [N,72,6,6] map, so every kernel selection is compared element by element at the stage it computes - last
rows and columns, tile seams, every channel group - instead of through the layers after it.  "proj" is the natural network.

Exact-fp32 arithmetic: every router operation is x 1 (the projection: x a power of two) and + 0, so the output IS the stage's
fp32 value; |got - want| <= 4 r32 a[e] per element, with a[e] the element's magnitude bound (stage_cases.magnitude) and r32 the
fp32 ORACLE's own largest |fp32 - fp64| / a at that stage, recomputed here - never a figure of the GPU's.
Split-fp16 arithmetic: relative to the stage's largest reference magnitude in the call, BAND_TOL + k 2^-21 with k the number of
shortcut routers after the stage (two split convolutions each, 2^-22 of the element each).

Time on the MI355X: one HipEngine construction 0.05 - 0.09 s; one case (8 handles, 9 backbone calls and one built-in calibration
each) 0.4 - 1.0 s, "proj" 0.1 s.

Measured on the MI355X, worst over a stage's handles.  r32: the fp32 oracle's figure, here and on the GPU machine's CPU (it is
oneDNN's rounding: another CPU or thread count may give another figure, and the allowance moves with it).  fp32 / latency: max
|got - want| / (r32 a[e]), default mode (block fusion off: the same bits everywhere) / latency mode on 2 crops; allowed 4, or 8
where FP32_MARGIN_AT says so.  split: max |got - want| / max |want|, dynamic scales with resident weights 1, 0, 4, 5, then
calibrated; allowed 3e-6 + k 2^-21.
  stage        r32      fp32  latency  split dynamic 1 / 0 / 4 / 5                calibrated
  stem         2.24e-7  0.78  0.78     2.64e-7  2.64e-7  2.64e-7  2.64e-7         2.67e-7
  layers.1.0   2.58e-8  2.77  1.97     6.12e-7  6.12e-7  6.12e-7  6.12e-7         6.29e-7
  layers.1.1   4.25e-8  5.06  2.09     7.79e-7  7.79e-7  7.79e-7  7.79e-7         1.03e-6
  layers.2.0   5.40e-8  2.76  1.61     6.33e-7  6.33e-7  7.86e-7  6.33e-7         6.64e-7
  layers.2.1   4.05e-8  4.12  1.32     5.99e-7  6.53e-7  1.01e-6  6.53e-7         8.07e-7
  layers.2.2   4.08e-8  4.60  1.45     6.86e-7  6.82e-7  1.26e-6  6.82e-7         8.30e-7
  layers.3.0   3.71e-8  3.66  1.39     6.02e-7  6.02e-7  9.50e-7  6.02e-7         8.96e-7
  layers.3.1   2.39e-8  4.72  1.64     6.33e-7  6.22e-7  9.21e-7  6.22e-7         7.81e-7
  layers.3.2   2.36e-8  5.24  1.73     7.36e-7  7.64e-7  1.01e-6  7.64e-7         8.00e-7
  layers.3.3   2.95e-8  4.44  1.25     7.12e-7  7.12e-7  1.10e-6  7.12e-7         8.49e-7
  layers.3.4   2.25e-8  7.28  1.72     1.00e-6  9.72e-7  1.18e-6  9.72e-7         9.03e-7
  layers.4.0   2.20e-8  4.29  1.10     7.06e-7  6.89e-7  8.29e-7  6.89e-7         6.35e-7
  layers.4.1   2.88e-8  3.39  0.85     7.19e-7  6.81e-7  9.70e-7  6.81e-7         6.70e-7
  proj         2.88e-7  3.47  0.88     7.97e-7  1.10e-6  1.02e-6  1.10e-6         8.98e-7
The all-zero router layers (zero weight rows, zero L1 bounds, all-zero activation tensors) gave no non-finite value and raised
nothing in any mode."""
import time

import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, synth

import stage_cases as sc
from test_gpu_split_range import BAND_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_MARGIN = 4.0        # over r32: the same products summed in another order with the same unit roundoff
# (stage, mode) -> margin where a correct kernel needs more than FP32_MARGIN: the next power of two above the measured figure.
# One reason for all of them, from conv_igemm.hip (layer1: conv_patch.hip, one 144-MFMA stream per tile): an accumulator starts at
# bias + residual and takes all K = 9 cin products one after another (K = 288 .. 2304), while r32 is the rounding of the oracle's oneDNN convolution, which keeps several partial sums
# and rounds less than one K-long chain.  oracle/studies/fp32_chain.py runs that plain chain on the CPU in the kernel's k order:
# 4.50 at layers.1.1, 4.06 / 3.48 at 2.1 / 2.2, 4.78 / 4.72 / 4.90 / 8.09 at 3.1 .. 3.4, 4.65 at 4.0 (x r32 a[e]) - the
# stages and sizes seen on the GPU (5.06; 4.12 / 4.60; 4.72 / 5.24 / 4.44 / 7.28; 4.29).  Latency mode walks K in several shorter
# chains (split-K) and stays below 2.1.  Block fusion off has the default mode's bits, so both modes carry the entry.
FP32_MARGIN_AT = {(stage, mode): 8.0
                  for stage in ("_layers.1.1", "_layers.2.1", "_layers.2.2", "_layers.3.1", "_layers.3.2", "_layers.3.3",
                                "_layers.3.4", "_layers.4.0")
                  for mode in ("fp32", "fp32_unfused")}
RESIDENT = (1, 0, 4, 5)  # conv_w4 | chunked conv_split | conv_c64k on layer2 | conv_w4 on layer3/4, chunked layer2


@pytest.fixture(scope="module")
def net():
    sd = synth.synthetic_state_dict(0)
    return (sd,) + sc.references(sd)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fp32_ratio(got, want, a, r32):
    """max_e |got - want| / (r32 a[e]); inf where a[e] == 0 and got != 0."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    zero = a == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return (err / (r32 * a.clamp_min(1e-300)))[~zero].max().item()


def _split_rel(got, want, scale):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    return (got - want).abs().max().item() / scale


def _run_handle(rsd, x, want, a, r32, stage_max, figures):
    """One handle in every mode; the worst figure per mode is merged into `figures`."""
    def note(mode, v):
        figures[mode] = max(figures.get(mode, 0.0), v)
    n_lat, n_cal = 2, sc.N_SYNTH
    t0 = time.perf_counter()
    eng = _native.HipEngine(rsd, DEV)
    figures["create_s"] = max(figures.get("create_s", 0.0), time.perf_counter() - t0)
    try:
        # ---- exact fp32: streaming 1x1 launches (default), one conv_igemm launch per layer, split-K on two crops
        fused = eng.backbone(x)
        note("fp32", _fp32_ratio(fused, want, a, r32))
        eng.set_block_fusion(False)
        plain = eng.backbone(x)
        note("fp32_unfused", _fp32_ratio(plain, want, a, r32))
        assert torch.equal(fused, plain), "block fusion changes fp32 bits"
        eng.set_block_fusion(True)
        eng.set_latency_mode(True)
        note("fp32_latency", _fp32_ratio(eng.backbone(x[:n_lat]), want[:n_lat], a[:n_lat], r32))
        eng.set_latency_mode(False)
        eng.poll_status()
        # ---- split fp16, dynamic scales, every kernel selection
        eng.set_split_scale("dynamic")
        eng.set_conv_arithmetic("split_f16_always")
        for resident in RESIDENT:
            eng.set_resident_weights(resident)
            got = eng.backbone(x)
            eng.poll_status()
            note(f"split_dynamic_{resident}", _split_rel(got, want, stage_max[0]))
        # ---- calibrated scales (the built-in calibration set, on this network), the synthetic crops only
        eng.set_resident_weights(1)
        eng.set_split_scale("calibrated")
        got = eng.backbone(x[:n_cal])
        eng.poll_status()
        note("split_calibrated", _split_rel(got, want[:n_cal], stage_max[1]))
    finally:
        eng.close()


@pytest.mark.parametrize("stage", sc.STAGES + ["proj"])
def test_stage_against_fp64(net, stage):
    """Every handle of the stage's plan, 6 crops (3 synthetic, constant 1, corner pixels, checkerboard) in one call per mode.
    fp32 modes (default, block fusion off - also bit-equal to the default through every router -, latency mode on 2 crops):
    |got - want| <= 4 r32 a[e], 0 where a[e] = 0.  Split-fp16, dynamic scales with resident weights 1, 0, 4, 5, and calibrated
    scales on the 3 synthetic crops: finite, poll_status clean, within BAND_TOL + k 2^-21 of the stage's largest.
    The measured figures of every stage and mode are in the module docstring."""
    sd, crops, t64, _t32, a_all, r32_all = net
    x = _dev(crops)
    k = 0 if stage == "proj" else len(sc.stage_geometry(stage)[2])
    split_tol = BAND_TOL + k * 2.0 ** -21
    stage_max = (t64[stage].abs().max().item(), t64[stage][: sc.N_SYNTH].abs().max().item())
    figures = {}
    t0 = time.perf_counter()
    if stage == "proj":
        _run_handle(sd, x, t64[stage], a_all[stage], r32_all[stage], stage_max, figures)
    else:
        for offsets, chan0 in sc.router_plan(stage):
            rsd, sel = sc.router_state_dict(sd, stage, offsets, chan0)
            _run_handle(rsd, x, sc.gather(t64[stage], sel), sc.gather(a_all[stage], sel), r32_all[stage], stage_max, figures)
    print(f"\n{stage}: r32 {r32_all[stage]:.3g} case {time.perf_counter() - t0:.2f} s",
          " ".join(f"{m}:{v:.3g}" for m, v in figures.items()))
    for mode, v in figures.items():
        if mode.startswith("fp32"):
            assert v <= FP32_MARGIN_AT.get((stage, mode), FP32_MARGIN), (stage, mode, v)
        elif mode.startswith("split"):
            assert v <= split_tol, (stage, mode, v, split_tol)
