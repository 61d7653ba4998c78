"""Time ut_smooth_pose_sequence (csrc/smooth.hip) with device events on two workloads: 4096 sequences x 16 frames, the
sliding-window shape, and 2 x 369, one recording of two hands.  The frames are the 74 golden hands of tests/views_cases.py
golden() repeated - the pose at tracking starts (tests/robust_cases.py tracking_starts), pose_info and pivot what
ut_pose_information_views gives at those poses in their two seeing views - so consecutive frames differ by far more than a hand
moves: the smoother's arithmetic does not depend on the values, only the timing is read.  With and without param_sigma.

The yardsticks are ut_pose_information_views and ut_fit_pose_views on the same number of poses, measured in the same run: the timed
windows of all launches of a workload are interleaved - one window of each in turn, after five warm-up launches each - so that a
drift of the device's clock meets all of them alike.  Prints one JSON line per case: microseconds per launch (median of --repeats
windows of --iters launches, and their spread), and for the smoother the ratio to each yardstick's median.  No threshold is set.

    python tools/bench_smooth.py [--iters 50] [--repeats 7]
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
import smooth_cases as sm  # noqa: E402
import views_cases as vc  # noqa: E402
from absolutetrack_amd import _native  # noqa: E402
from bench_views import interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = vc.golden()
    hm = g["hm"]
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    c = vc.case("two_views")
    table = torch.from_numpy(c["table"]).to(dev)
    step_var = torch.from_numpy(sm.step_var()).reshape(1, 26).to(dev)
    for n_seq, frames in ((4096, 16), (2, 369)):
        n = n_seq * frames
        idx = np.arange(n) % 74
        ja0, xf0 = rc.tracking_starts(dict(ja=g["ja"][idx], xf=g["xf"][idx]), 0)
        ja0, xf0 = torch.from_numpy(ja0).to(dev), torch.from_numpy(xf0).to(dev)
        mirror = torch.from_numpy(g["hand"][idx]).to(dev)
        win, rows, weights = (torch.from_numpy(c[f][idx]).to(dev) for f in ("window", "cam_rows", "weights"))
        fit_out, fit_info = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)), torch.empty(n, 4, device=dev)
        cov = dict(pose_info=torch.empty(n, 351, device=dev), pivot=torch.empty(n, 3, device=dev), param_sigma=False, landmark_cov=False,
                   info=torch.empty(n, 4, device=dev))
        information = lambda: _native.pose_information_views(blob, ja0, xf0, win, rows, table, weights=weights, mirror=mirror, **cov)
        information()
        work = torch.empty(n, _native.UT_SMOOTH_WORK, device=dev)
        out = (torch.empty(n_seq, frames, 22, device=dev), torch.empty(n_seq, frames, 4, 4, device=dev))
        sigma, info = torch.empty(n_seq, frames, 26, device=dev), torch.empty(n_seq, frames, 4, device=dev)
        poses = (ja0.reshape(n_seq, frames, 22), xf0.reshape(n_seq, frames, 4, 4), cov["pose_info"], cov["pivot"], step_var)

        def smooth(with_sigma):
            return lambda: _native.smooth_pose_sequence(*poses, out=out, param_sigma=sigma if with_sigma else False, info=info, workspace=work)

        fns = {"fit": lambda: _native.fit_pose_views(blob, win, rows, table, ja0, xf0, weights=weights, mirror=mirror, out=fit_out, info=fit_info),
               "information": information, "smooth": smooth(False), "smooth_sigma": smooth(True)}
        t = interleaved(fns, args.iters, args.repeats)
        status = info.cpu().numpy()[..., 3]
        for name, entry in (("fit", "fit_pose_views"), ("information", "pose_information_views")):
            us, lo, hi = t[name]
            print(json.dumps({"bench": entry, "poses": n, "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                              "yardstick_spread": round((hi - lo) / us, 4)}), flush=True)
        for name in ("smooth", "smooth_sigma"):
            us, lo, hi = t[name]
            print(json.dumps({"bench": f"smooth_pose_sequence{'_with_sigma' if name == 'smooth_sigma' else ''}", "sequences": n_seq, "frames": frames,
                              "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                              "over_pose_information_views": round(us / t["information"][0], 4), "over_fit_pose_views": round(us / t["fit"][0], 4),
                              "ok_fraction": round(float(((status.astype(np.int64) & 1) == 1).mean()), 4)}), flush=True)


if __name__ == "__main__":
    main()
