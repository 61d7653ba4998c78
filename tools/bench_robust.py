"""Time ut_fit_pose_views_robust (csrc/fit_views_robust.hip) with device events: 512, 2048 and 8192 hands - the 74 hands of
tests/views_cases.py golden() repeated, their two seeing views, the reference's own windows, tracking starts +-0.05 rad on the 20
angles and the wrist's rotation / +-5 mm (tests/robust_cases.py tracking_starts, drawn per copy, so that no two copies are the same
problem) - under Huber and Geman-McClure at 3 px, on the clean windows and with 2 detections per view displaced by 40 px.  Prints
one JSON line per case: microseconds per launch (median of --repeats windows of --iters launches, and their spread), mean and
largest iteration count, microseconds per iteration (per launch / mean iterations), the fraction converged.

The yardstick is ut_fit_pose_views (csrc/fit_views.hip, device code unchanged) on the same hands and starts with the clean
windows.  The timed windows of the five launches are interleaved - one window of each in turn - so that a drift of the device's
clock meets all of them alike; `per_iteration_over_fit_pose_views` is the ratio of the times per iteration - what the weight psi
costs -, `over_fit_pose_views` of the medians per launch, and `yardstick_spread` the yardstick's own (max - min) / median, the
margin a ratio has to leave before it says anything.  No threshold is set.

    python tools/bench_robust.py [--iters 50] [--repeats 7]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import robust_cases as rc  # noqa: E402
import views_cases as vc  # noqa: E402
from absolutetrack_amd import _native  # noqa: E402
from bench_views import interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = vc.golden()
    hm = g["hm"]
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    table = torch.from_numpy(g["table"]).to(dev)
    two = vc.select(g, g["seeing"])
    for n in (512, 2048, 8192):
        idx = np.arange(n) % 74
        clean = dict(table=g["table"], **{f: two[f][idx] for f in ("window", "cam_rows", "weights")})
        dirty = rc.contaminated(clean, rc.OUTLIERS, rc.OUTLIER_PX, 0)
        ja0, xf0 = rc.tracking_starts(dict(ja=g["ja"][idx], xf=g["xf"][idx]), 0)
        ja0, xf0 = torch.from_numpy(ja0).to(dev), torch.from_numpy(xf0).to(dev)
        mirror = torch.from_numpy(g["hand"][idx]).to(dev)
        rows, weights = torch.from_numpy(clean["cam_rows"]).to(dev), torch.from_numpy(clean["weights"]).to(dev)
        win = {"clean": torch.from_numpy(clean["window"]).to(dev), "dirty": torch.from_numpy(dirty["window"]).to(dev)}
        cases = [("views", "fit_pose_views_clean", None, "clean")] + \
                [(f"{loss}_{w}", f"fit_pose_views_robust_{loss}_{w}", loss, w) for loss in rc.ROBUST for w in ("clean", "dirty")]
        outs = {k: (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)) for k, *_ in cases}
        infos = {k: torch.empty(n, 4, device=dev) for k in outs}

        def launch(k, loss, w):
            if loss is None:
                return lambda: _native.fit_pose_views(blob, win[w], rows, table, ja0, xf0, weights=weights, mirror=mirror, out=outs[k], info=infos[k])
            return lambda: _native.fit_pose_views_robust(blob, win[w], rows, table, ja0, xf0, weights=weights, mirror=mirror, loss=loss,
                                                         loss_scale=rc.SCALE_PX, out=outs[k], info=infos[k])

        t = interleaved({k: launch(k, loss, w) for k, _name, loss, w in cases}, args.iters, args.repeats)
        result = {}
        for k, name, _loss, _w in cases:
            us, lo, hi = t[k]
            r = infos[k].cpu().numpy()
            result[k] = {"bench": name, "poses": n, "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                         "mean_iterations": round(float(r[:, 2].mean()), 2), "max_iterations": int(r[:, 2].max()),
                         "us_per_iteration": round(us / float(r[:, 2].mean()), 2),
                         "converged_fraction": round(float((r[:, 3].astype(int) & 1).astype(bool).mean()), 4)}
        result["views"]["yardstick_spread"] = round((t["views"][2] - t["views"][1]) / t["views"][0], 4)
        for k in result:
            if k != "views":
                result[k]["over_fit_pose_views"] = round(result[k]["us_per_launch"] / result["views"]["us_per_launch"], 3)
                result[k]["per_iteration_over_fit_pose_views"] = round(result[k]["us_per_iteration"] / result["views"]["us_per_iteration"], 3)
        for row in result.values():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
