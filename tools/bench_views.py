"""Time ut_fit_pose_views (csrc/fit_views.hip) with device events: 512, 2048 and 8192 hands - the 74 hands of
tests/views_cases.py golden() repeated, their two seeing views and their best view alone, the reference's own windows, warm
starts +-0.1 rad on the 20 angles / +-10 mm on the wrist (default_rng(0), drawn per copy, so that no two copies are the same
problem).  Prints one JSON line per case: microseconds per launch (median of --repeats windows of --iters launches, and their
spread), mean and largest iteration count, microseconds per iteration (per launch / mean iterations).

The yardstick is ut_fit_pose_info (csrc/fit_info.hip, unchanged), warm from the same starts on the same hands - targets and
factors from ut_triangulate_points_info of the two views.  The timed windows of the three launches are interleaved - one
window of each in turn - so that a drift of the device's clock meets all of them alike; `over_fit_pose_info` is the ratio of
the medians per launch, `per_iteration_over_fit_pose_info` of the times per iteration, and `yardstick_spread` the yardstick's
own (max - min) / median, the margin a ratio has to leave before it says anything.

    python tools/bench_views.py [--iters 50] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import views_cases as vc  # noqa: E402
from absolutetrack_amd import _native  # noqa: E402


def interleaved(fns, iters, repeats):
    """{name: (median, min, max) us per launch}: one timed window of every function in turn, `repeats` rounds."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (float(np.median(t)), min(t), max(t)) for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_views.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = vc.golden()
    hm = g["hm"]
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    table = torch.from_numpy(g["table"]).to(dev)
    two, one = vc.select(g, g["seeing"]), vc.select(g, g["best"])
    for n in (512, 2048, 8192):
        idx = np.arange(n) % 74
        rng = np.random.default_rng(0)
        ja0 = g["ja"][idx].copy()
        ja0[:, :20] += rng.uniform(-0.1, 0.1, (n, 20))
        xf0 = g["xf"][idx].copy()
        xf0[:, :3, 3] += rng.uniform(-10.0, 10.0, (n, 3))
        ja0, xf0 = torch.from_numpy(ja0.astype(np.float32)).to(dev), torch.from_numpy(xf0.astype(np.float32)).to(dev)
        mirror = torch.from_numpy(g["hand"][idx]).to(dev)
        dv = {k: {f: torch.from_numpy(c[f][idx]).to(dev) for f in ("window", "cam_rows", "weights")} for k, c in (("two", two), ("one", one))}
        kp = torch.empty(n, 21, 3, device=dev)
        factor = _native.triangulate_points_info(dv["two"]["window"], dv["two"]["cam_rows"], table, weights=dv["two"]["weights"],
                                                 out_f32=kp, point_stride=63)[3]
        outs = {k: (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)) for k in ("info", "two", "one")}
        infos = {k: torch.empty(n, 4, device=dev) for k in outs}

        def fit_pose_info():
            _native.fit_pose_info(blob, kp, factor, init_angles=ja0, init_wrist_xf=xf0, mirror=mirror, out=outs["info"], info=infos["info"])

        def views(k):
            return lambda: _native.fit_pose_views(blob, dv[k]["window"], dv[k]["cam_rows"], table, ja0, xf0, weights=dv[k]["weights"],
                                                  mirror=mirror, out=outs[k], info=infos[k])

        t = interleaved({"info": fit_pose_info, "two": views("two"), "one": views("one")}, args.iters, args.repeats)
        rows = {}
        for k, name in (("info", "fit_pose_info_warm"), ("two", "fit_pose_views_two_views"), ("one", "fit_pose_views_one_view")):
            us, lo, hi = t[k]
            r = infos[k].cpu().numpy()
            rows[k] = {"bench": name, "poses": n, "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                       "mean_iterations": round(float(r[:, 2].mean()), 2), "max_iterations": int(r[:, 2].max()),
                       "us_per_iteration": round(us / float(r[:, 2].mean()), 2),
                       "converged_fraction": round(float((r[:, 3].astype(int) & 1).astype(bool).mean()), 4)}
        spread = (t["info"][2] - t["info"][1]) / t["info"][0]
        rows["info"]["yardstick_spread"] = round(spread, 4)
        for k in ("two", "one"):
            rows[k]["over_fit_pose_info"] = round(rows[k]["us_per_launch"] / rows["info"]["us_per_launch"], 3)
            rows[k]["per_iteration_over_fit_pose_info"] = round(rows[k]["us_per_iteration"] / rows["info"]["us_per_iteration"], 3)
        for row in rows.values():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
