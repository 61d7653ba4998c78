"""Time ut_start_pose_views and ut_select_pose (csrc/start_views.hip) with device events: 2048 hands x 4 bank poses x 24 seeds x 30
rounds, in the two seeing views and in the best view alone.  The hands are the 74 golden hands of tests/views_cases.py golden()
repeated, with the reference's own windows.

The yardsticks are ut_fit_pose_views on the same 2048 hands from tracking starts (tests/robust_cases.py tracking_starts) - one warm
fit per hand, what a tracker pays anyway - and on the 8192 starts the kernel wrote, measured in the same run: the timed windows of all
launches of a workload are interleaved - one window of each in turn, after five warm-up launches each - so that a drift of the
device's clock meets all of them alike.  Prints one JSON line per launch: microseconds (median of --repeats windows of --iters
launches, and their spread), and the cold chain - start + fit of the 8192 starts + selection - as a multiple of the warm fit.  No
threshold is set.

    python tools/bench_start.py [--iters 20] [--repeats 7]
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
import start_cases as sc  # noqa: E402
import views_cases as vc  # noqa: E402
from absolutetrack_amd import _native  # noqa: E402
from bench_views import interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    ap.add_argument("--hands", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_start.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = vc.golden()
    hm = g["hm"]
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    bank, seeds = torch.from_numpy(sc.bank()).to(dev), torch.from_numpy(sc.seeds()).to(dev)
    n, k = args.hands, bank.shape[0]
    idx = np.arange(n) % 74
    for views in ("two", "one"):
        c = sc.golden_case(views, 0)
        table = torch.from_numpy(c["table"]).to(dev)
        win, rows, weights = (torch.from_numpy(c[f][idx]).to(dev) for f in ("window", "cam_rows", "weights"))
        mirror = torch.from_numpy(c["mirror"][idx]).to(dev)
        ja0, xf0 = rc.tracking_starts(dict(ja=g["ja"][idx], xf=g["xf"][idx]), 0)
        ja0, xf0 = torch.from_numpy(ja0).to(dev), torch.from_numpy(xf0).to(dev)
        starts, start_info = (torch.empty(n * k, 22, device=dev), torch.empty(n * k, 4, 4, device=dev)), torch.empty(n * k, 4, device=dev)
        warm_out, warm_info = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)), torch.empty(n, 4, device=dev)
        fit_out, fit_info = (torch.empty(n * k, 22, device=dev), torch.empty(n * k, 4, 4, device=dev)), torch.empty(n * k, 4, device=dev)
        sel_out, sel_info, sel_index = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)), torch.empty(n, 4, device=dev), \
            torch.empty(n, dtype=torch.int32, device=dev)
        win_k, rows_k, weights_k, mirror_k = (t.repeat_interleave(k, 0) for t in (win, rows, weights, mirror))
        start = lambda: _native.start_pose_views(blob, win, rows, table, bank, seeds, weights, None, mirror, iters=sc.ITERS, out=starts, info=start_info)
        start()
        fns = {"start": start,
               "warm_fit": lambda: _native.fit_pose_views(blob, win, rows, table, ja0, xf0, weights=weights, mirror=mirror, out=warm_out, info=warm_info),
               "fit_of_starts": lambda: _native.fit_pose_views(blob, win_k, rows_k, table, starts[0], starts[1], weights=weights_k, mirror=mirror_k,
                                                               out=fit_out, info=fit_info),
               "select": lambda: _native.select_pose(fit_out[0], fit_out[1], fit_info, k, out=sel_out, out_info=sel_info, out_index=sel_index)}
        t = interleaved(fns, args.iters, args.repeats)
        its = fit_info.cpu().numpy()[:, 2]
        for name, what in (("start", "start_pose_views"), ("warm_fit", "fit_pose_views"), ("fit_of_starts", "fit_pose_views_on_starts"), ("select", "select_pose")):
            us, lo, hi = t[name]
            print(json.dumps({"bench": what, "views": views, "hands": n, "rows": n * k if name in ("start", "fit_of_starts") else n,
                              "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1)}), flush=True)
        chain = t["start"][0] + t["fit_of_starts"][0] + t["select"][0]
        print(json.dumps({"bench": "cold_chain", "views": views, "hands": n, "bank": k, "seeds": int(seeds.shape[0]), "rounds": sc.ITERS,
                          "us": round(chain, 1), "over_warm_fit": round(chain / t["warm_fit"][0], 3),
                          "start_over_warm_fit": round(t["start"][0] / t["warm_fit"][0], 3),
                          "fit_iterations_mean_from_starts": round(float(its.mean()), 2),
                          "refused_starts": int((start_info[:, 3] != 0).sum()), "chosen_refused": int((sel_index < 0).sum())}), flush=True)


if __name__ == "__main__":
    main()
