"""Time ut_fit_pose_scale and ut_pool_scale (csrc/fit_scale.hip) with device events: 512, 2048 and 8192 poses of the
recording's labels, exact targets, cold start.  Prints one JSON line per case: microseconds per launch (median of --repeats
windows of --iters launches), mean and largest iteration count, microseconds per iteration (per launch / mean iterations).
The yardstick is ut_fit_pose (csrc/fit.hip, unchanged) on the same targets and starts: `per_iteration_over_fit_pose` is the
free pass's time per iteration over ut_fit_pose's.  Beside it the fixed pass (warm-started from the free pass, at its scales),
the pool alone (groups of 64) and the chain free pass -> pool -> fixed pass that hand.calibrate_scale launches.

    python tools/bench_scale.py [--iters 50] [--repeats 7]
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

import fit_cases as fc  # noqa: E402
import mesh_cases as mc  # noqa: E402
from absolutetrack_amd import _native, pipeline  # noqa: E402
from bench_fit import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scale.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja_all, xf_all, hand_all = mc.label_poses(lab)
    targets_all = fc.forward(hm, ja_all, fc.effective_wrist(xf_all, hand_all, 1.0, np.float64))
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    for n in (512, 2048, 8192):
        idx = np.arange(n) % ja_all.shape[0]
        targets = torch.from_numpy(targets_all[idx]).float().to(dev)
        mirror = torch.from_numpy(hand_all[idx]).to(dev)
        out = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        out2 = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        info4, info, info2 = torch.empty(n, 4, device=dev), torch.empty(n, 6, device=dev), torch.empty(n, 6, device=dev)
        scale, scale2, pose_scale = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
        group = torch.empty(n // 64, 4, device=dev)

        def fit_pose():
            _native.fit_pose(blob, targets, mirror=mirror, out=out, info=info4)

        def free():
            _native.fit_pose_scale(blob, targets, mirror=mirror, out=out, scale=scale, info=info)

        def pool():
            _native.pool_scale(scale, info, 64, group=group, pose_scale=pose_scale)

        def fixed():
            _native.fit_pose_scale(blob, targets, init_scale=pose_scale, scale_mode=_native.UT_SCALE_FIXED, init_angles=out[0],
                                   init_wrist_xf=out[1], mirror=mirror, out=out2, scale=scale2, info=info2)

        def chain():
            free()
            pool()
            fixed()

        rows = {}
        for name, fn, res in (("fit_pose", fit_pose, info4), ("fit_pose_scale_free", free, info), ("pool_scale", pool, None),
                              ("fit_pose_scale_fixed_warm", fixed, info2), ("free_pool_fixed_chain", chain, None)):
            us, lo, hi = timed(fn, args.iters, args.repeats)
            row = {"bench": name, "poses": n, "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1)}
            if res is not None:
                r = res.cpu().numpy()
                row.update(mean_iterations=round(float(r[:, 2].mean()), 2), max_iterations=int(r[:, 2].max()),
                           us_per_iteration=round(us / float(r[:, 2].mean()), 2),
                           converged_fraction=round(float((r[:, 3].astype(int) & 1).astype(bool).mean()), 4))
            rows[name] = row
        rows["fit_pose_scale_free"]["per_iteration_over_fit_pose"] = round(
            rows["fit_pose_scale_free"]["us_per_iteration"] / rows["fit_pose"]["us_per_iteration"], 3)
        rows["fit_pose_scale_free"]["per_launch_over_fit_pose"] = round(
            rows["fit_pose_scale_free"]["us_per_launch"] / rows["fit_pose"]["us_per_launch"], 3)
        for row in rows.values():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
