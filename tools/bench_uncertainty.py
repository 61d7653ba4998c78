"""Time ut_pose_information_views (csrc/pose_info_views.hip) with device events on 8192 hands - the 74 hands of
tests/views_cases.py golden() repeated, their two seeing views, exact windows of the label poses (views_cases.case "two_views" for
the Fisheye62 cameras, "pinhole" for pinhole ones), the pose at tracking starts +-0.05 rad on the 20 angles and the wrist's
rotation / +-5 mm (tests/robust_cases.py tracking_starts, drawn per copy) - for both camera kinds and the three losses (3 px).

The yardstick is ut_fit_pose_views (csrc/fit_views.hip) on the same inputs, from the same poses as its starts, measured in the same
run: the timed windows of the launches of one camera kind are interleaved - one window of each in turn, after five warm-up
launches each - so that a drift of the device's clock meets all of them alike.  Prints one JSON line per case: microseconds per
launch (median of --repeats windows of --iters launches, and their spread), and for the information launches `over_fit_pose_views`,
the ratio of the medians, next to the yardstick's own spread (max - min) / median, the margin a ratio has to leave before it says
anything, and the fit's mean iteration count.  No threshold is set.

    python tools/bench_uncertainty.py [--poses 8192] [--iters 50] [--repeats 7]
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
    ap.add_argument("--poses", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = vc.golden()
    hm = g["hm"]
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    n = args.poses
    idx = np.arange(n) % 74
    ja0, xf0 = rc.tracking_starts(dict(ja=g["ja"][idx], xf=g["xf"][idx]), 0)
    ja0, xf0 = torch.from_numpy(ja0).to(dev), torch.from_numpy(xf0).to(dev)
    mirror = torch.from_numpy(g["hand"][idx]).to(dev)
    for kind, name in (("fisheye62", "two_views"), ("pinhole", "pinhole")):
        c = vc.case(name)
        table = torch.from_numpy(c["table"]).to(dev)
        win, rows, weights = (torch.from_numpy(c[f][idx]).to(dev) for f in ("window", "cam_rows", "weights"))
        fit_out, fit_info = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)), torch.empty(n, 4, device=dev)
        outs = {loss: dict(pose_info=torch.empty(n, 351, device=dev), pivot=torch.empty(n, 3, device=dev),
                           param_sigma=torch.empty(n, 26, device=dev), landmark_cov=torch.empty(n, 21, 6, device=dev),
                           info=torch.empty(n, 4, device=dev)) for loss in rc.LOSSES}

        def information(loss):
            return lambda: _native.pose_information_views(blob, ja0, xf0, win, rows, table, weights=weights, mirror=mirror, loss=loss,
                                                          loss_scale=rc.SCALE_PX, **outs[loss])

        fns = {"fit": lambda: _native.fit_pose_views(blob, win, rows, table, ja0, xf0, weights=weights, mirror=mirror, out=fit_out,
                                                     info=fit_info)}
        fns.update({loss: information(loss) for loss in rc.LOSSES})
        t = interleaved(fns, args.iters, args.repeats)
        iters = fit_info.cpu().numpy()[:, 2]
        us, lo, hi = t["fit"]
        print(json.dumps({"bench": f"fit_pose_views_{kind}", "poses": n, "us_per_launch": round(us, 1), "us_min": round(lo, 1),
                          "us_max": round(hi, 1), "mean_iterations": round(float(iters.mean()), 2),
                          "yardstick_spread": round((hi - lo) / us, 4)}), flush=True)
        for loss in rc.LOSSES:
            u, l, h = t[loss]
            status = outs[loss]["info"].cpu().numpy()[:, 3]
            print(json.dumps({"bench": f"pose_information_views_{kind}_{loss}", "poses": n, "us_per_launch": round(u, 1), "us_min": round(l, 1),
                              "us_max": round(h, 1), "over_fit_pose_views": round(u / us, 4),
                              "ok_fraction": round(float((status == _native.UT_COV_OK).mean()), 4)}), flush=True)


if __name__ == "__main__":
    main()
