"""Time ut_fit_pose_info (csrc/fit_info.hip) and the chain it ends with device events: 512, 2048 and 8192 hands - the 74 hands of
tests/triangulate_cases.py golden_case repeated, Gaussian noise of --noise px (default_rng(0)) on every window, so that no two
copies are the same problem.  Prints one JSON line per case: microseconds per launch (median of --repeats windows of --iters
launches), mean and largest iteration count, microseconds per iteration (per launch / mean iterations).  The yardstick is
ut_fit_pose (csrc/fit.hip, unchanged), cold on the same triangulated targets: `per_iteration_over_fit_pose` is the information
fit's time per iteration, warm-started from that isotropic result, over ut_fit_pose's.  Trip counts differ between those two (a
launch lasts as long as its slowest pose), so a third row runs ut_fit_pose_info cold with the factors I - ut_fit_pose's cost, hence
its path and trip counts - and `same_path_over_fit_pose` is the ratio of those two launches: what the whitening costs.  Beside
them the triangulation without and with the factor, and the chain triangulation with factor -> ut_fit_pose -> ut_fit_pose_info that
tracker.hand_pose_from_window_keypoints(use_information=True) launches.

    python tools/bench_info.py [--iters 50] [--repeats 7] [--noise 0.25]
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

import info_cases as ic  # noqa: E402
from absolutetrack_amd import _native  # noqa: E402
from bench_fit import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    ap.add_argument("--noise", type=float, default=0.25, help="px of Gaussian noise on the windows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_info.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = ic.golden_hands()
    hm = g["hm"]
    blob = torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"],
                                                    hm["landmark_rest_positions"], hm["landmark_rest_bone_weights"],
                                                    hm["landmark_rest_bone_indices"])).reshape(1, 321).to(dev)
    table = torch.from_numpy(g["table"]).to(dev)
    for n in (512, 2048, 8192):
        idx = np.arange(n) % 74
        window = g["window"][idx] + np.random.default_rng(0).normal(0.0, args.noise, (n, 4, 21, 2))
        window = torch.from_numpy(window).to(dev)
        rows = torch.from_numpy(g["cam_rows"][idx]).to(dev)
        weights = torch.from_numpy(g["weights"][idx]).to(dev)
        mirror = torch.from_numpy(g["hand"][idx]).to(dev)
        tri_out = (torch.empty(n, 21, 3, dtype=torch.float64, device=dev), torch.empty(n, 21, 4, device=dev),
                   torch.empty(n, 4, 21, device=dev), torch.empty(n, 21, 6, device=dev))
        kp = torch.empty(n, 21, 3, device=dev)
        iso = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        out = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        out_eye = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        info_iso, info, info_eye = torch.empty(n, 4, device=dev), torch.empty(n, 4, device=dev), torch.empty(n, 4, device=dev)
        eye = torch.from_numpy(ic.isotropic(np.ones((n, 21), np.float32))).to(dev)

        def triangulate():
            _native.triangulate_points(window, rows, table, weights=weights, out=tri_out[:3], out_f32=kp, point_stride=63)

        def triangulate_info():
            _native.triangulate_points_info(window, rows, table, weights=weights, out=tri_out, out_f32=kp, point_stride=63)

        def fit_pose():
            _native.fit_pose(blob, kp, mirror=mirror, out=iso, info=info_iso)

        def fit_pose_info():
            _native.fit_pose_info(blob, kp, tri_out[3], init_angles=iso[0], init_wrist_xf=iso[1], mirror=mirror, out=out, info=info)

        def fit_pose_info_identity():
            _native.fit_pose_info(blob, kp, eye, mirror=mirror, out=out_eye, info=info_eye)

        def chain():
            triangulate_info()
            fit_pose()
            fit_pose_info()

        rows_out = {}
        for name, fn, res in (("triangulate_points", triangulate, None), ("triangulate_points_info", triangulate_info, None),
                              ("fit_pose", fit_pose, info_iso), ("fit_pose_info_warm", fit_pose_info, info),
                              ("fit_pose_info_identity_cold", fit_pose_info_identity, info_eye),
                              ("triangulate_fit_fit_info_chain", chain, None)):
            us, lo, hi = timed(fn, args.iters, args.repeats)
            row = {"bench": name, "poses": n, "noise_px": args.noise, "us_per_launch": round(us, 1), "us_min": round(lo, 1),
                   "us_max": round(hi, 1)}
            if res is not None:
                r = res.cpu().numpy()
                row.update(mean_iterations=round(float(r[:, 2].mean()), 2), max_iterations=int(r[:, 2].max()),
                           us_per_iteration=round(us / float(r[:, 2].mean()), 2),
                           converged_fraction=round(float((r[:, 3].astype(int) & 1).astype(bool).mean()), 4))
            rows_out[name] = row
        rows_out["fit_pose_info_warm"]["per_iteration_over_fit_pose"] = round(
            rows_out["fit_pose_info_warm"]["us_per_iteration"] / rows_out["fit_pose"]["us_per_iteration"], 3)
        rows_out["fit_pose_info_warm"]["per_launch_over_fit_pose"] = round(
            rows_out["fit_pose_info_warm"]["us_per_launch"] / rows_out["fit_pose"]["us_per_launch"], 3)
        rows_out["fit_pose_info_identity_cold"]["same_path_over_fit_pose"] = round(
            rows_out["fit_pose_info_identity_cold"]["us_per_launch"] / rows_out["fit_pose"]["us_per_launch"], 3)
        for row in rows_out.values():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
