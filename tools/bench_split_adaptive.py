#!/usr/bin/env python3
"""Cost of the adaptive split-scale mode (HipEngine.set_split_scale("adaptive")) on the headline HotPath step.

bench.py's shard (1024 frames, 2048 hand-frames, u8 noise, synthetic weights, split_f16 arithmetic), timed in rounds of
--steps steps that alternate between the modes, median ms per step per mode:
  leg "in_band": the built-in calibration, "calibrated" against "adaptive" (nothing adapts: the same launches and bits);
  leg "all_adapted": a handle calibrated on synthetic crops 4096 x brighter than normal ones, so that normal frames fall below
    the band's floor and the launches adapt - "adaptive" against "dynamic".  (Crops / 4096 would not do it in this biased
    network: its biases then set the calibrated words, and normal frames stay in band.)
The adaptation counter of one step is printed per leg.  One JSON line.
  python tools/bench_split_adaptive.py [--steps 10 --rounds 7 --warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time_steps(hot, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        hot.step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _leg(eng, hot, batch, modes, args):
    """{mode: {"ms_per_step": median, "ms_rounds": [...], "adapted_per_step": n}} with the modes alternating round by round."""
    out = {m: {"ms_rounds": []} for m in modes}
    for m in modes:
        eng.set_split_scale(m)
        for _ in range(args.warmup):
            hot.step(batch)
        hot.check()
        eng.split_adaptations(reset=True)
        hot.step(batch)
        hot.check()
        out[m]["adapted_per_step"] = eng.split_adaptations(reset=True)
    for r in range(args.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            eng.set_split_scale(m)
            hot.step(batch)                     # one untimed step after the switch
            out[m]["ms_rounds"].append(round(_time_steps(hot, batch, args.steps), 4))
    hot.check()
    for m in modes:
        out[m]["ms_per_step"] = statistics.median(out[m]["ms_rounds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from absolutetrack_amd import _native, pipeline, synth
    device = torch.device("cuda", 0)
    lab = pipeline.load_labels()
    hm = pipeline.hand_model_from_labels(lab)
    plan = {k: v.cpu().numpy() for k, v in pipeline.crop_plan_on_device(lab, hm, range(args.frames), device).items()}
    gen = torch.Generator(device=device)
    gen.manual_seed(1234)
    src = torch.randint(0, 256, (args.frames * 4, 480, 636), dtype=torch.uint8, device=device, generator=gen)
    batch = pipeline.make_batch(plan, src, device)
    res = {"hand_frames": batch.n_samples}

    eng = _native.HipEngine(synth.synthetic_state_dict(0), device)
    eng.set_conv_arithmetic("split_f16")
    res["in_band"] = _leg(eng, pipeline.HotPath(eng, hm, known_skeleton=True), batch, ["calibrated", "adaptive"], args)
    a, c = res["in_band"]["adaptive"]["ms_per_step"], res["in_band"]["calibrated"]["ms_per_step"]
    res["in_band"]["adaptive_over_calibrated"] = round(a / c, 4)
    eng.close()

    eng = _native.HipEngine(synth.synthetic_state_dict(0), device)
    eng.set_conv_arithmetic("split_f16")
    eng.calibrate_split(torch.from_numpy(synth.synthetic_crops(64, seed=5) * np.float32(4096.0)).to(device))
    res["all_adapted"] = _leg(eng, pipeline.HotPath(eng, hm, known_skeleton=True), batch, ["adaptive", "dynamic"], args)
    a, d = res["all_adapted"]["adaptive"]["ms_per_step"], res["all_adapted"]["dynamic"]["ms_per_step"]
    res["all_adapted"]["adaptive_over_dynamic"] = round(a / d, 4)
    res["all_adapted"]["adaptive_over_in_band_calibrated"] = round(a / c, 4)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
