"""Time ut_fit_pose (csrc/fit.hip) with device events: 512, 2048 and 8192 poses of the recording's labels, from the cold start
(exact targets) and from a warm start (labels perturbed by +-0.1 rad and +-10 mm, the size of a frame-to-frame move).
Prints one JSON line per case: microseconds per launch (median of --repeats windows), poses per second, mean and largest
iteration count, the share of poses that report convergence.  A new capability has no earlier time to compare with, so two
yardsticks stand beside each row:
  fk_floor_us   ut_fk on the same poses x the mean iteration count: every iteration evaluates the forward function once,
                so no solver built on ut_fk's arithmetic can be faster than that
  and, once, the float64 numpy solver of tests/fit_cases.py on the 738 label poses (host clock): the CPU baseline.

    python tools/bench_fit.py [--iters 50] [--repeats 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fit_cases as fc  # noqa: E402
import mesh_cases as mc  # noqa: E402
from absolutetrack_amd import _native, pipeline  # noqa: E402


def timed(fn, iters, repeats):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    ap.add_argument("--no-cpu", action="store_true", help="leave the numpy baseline out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja_all, xf_all, hand_all = mc.label_poses(lab)
    targets_all = fc.forward(hm, ja_all, fc.effective_wrist(xf_all, hand_all, 1.0, np.float64))
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    rng = np.random.default_rng(0)
    for n in (512, 2048, 8192):
        idx = np.arange(n) % ja_all.shape[0]
        targets = torch.from_numpy(targets_all[idx]).float().to(dev)
        mirror = torch.from_numpy(hand_all[idx]).to(dev)
        ja0 = ja_all[idx].copy()
        ja0[:, :20] += rng.uniform(-0.1, 0.1, (n, 20))
        xf0 = xf_all[idx].copy()
        xf0[:, :3, :3] = fc._rodrigues(rng.uniform(-0.1, 0.1, (n, 3))) @ xf0[:, :3, :3]
        xf0[:, :3, 3] += rng.uniform(-10, 10, (n, 3))
        warm = (torch.from_numpy(ja0).float().to(dev), torch.from_numpy(xf0).float().to(dev))
        label_ja, label_xf = torch.from_numpy(ja_all[idx]).float().to(dev), torch.from_numpy(xf_all[idx]).float().to(dev)
        out = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        info = torch.empty(n, 4, device=dev)
        fk_out = torch.empty(n, 21, 3, device=dev)
        fk_us, _lo, _hi = timed(lambda: _native._fk(_native.load_library(), None, dev, "stateless", blob, label_ja, label_xf,
                                                    mirror, 1.0, out=fk_out), args.iters, args.repeats)
        for start, init in (("cold", (None, None)), ("warm", warm)):
            def run():
                _native.fit_pose(blob, targets, init_angles=init[0], init_wrist_xf=init[1], mirror=mirror, out=out, info=info)
            us, lo, hi = timed(run, args.iters, args.repeats)
            res = info.cpu().numpy()
            its = res[:, 2]
            print(json.dumps({"bench": "fit_pose", "poses": n, "start": start, "us_per_launch": round(us, 1), "us_min": round(lo, 1),
                              "us_max": round(hi, 1), "poses_per_s": round(n / (us * 1e-6)), "mean_iterations": round(float(its.mean()), 2),
                              "max_iterations": int(its.max()),
                              "converged_fraction": round(float((res[:, 3].astype(int) & _native.UT_FIT_CONVERGED).astype(bool).mean()), 4),
                              "fk_us_per_launch": round(fk_us, 2), "fk_floor_us": round(fk_us * float(its.mean()), 1),
                              "times_the_fk_floor": round(us / (fk_us * float(its.mean())), 1)}), flush=True)
    if not args.no_cpu:
        t0 = time.perf_counter()
        _ja, _xf, info64 = fc.fit(hm, targets_all, mirror=hand_all)
        dt = time.perf_counter() - t0
        print(json.dumps({"bench": "fit_pose_numpy_float64", "poses": int(targets_all.shape[0]), "start": "cold", "seconds": round(dt, 3),
                          "poses_per_s": round(targets_all.shape[0] / dt), "mean_iterations": round(float(info64[:, 2].mean()), 2)}),
              flush=True)


if __name__ == "__main__":
    main()
