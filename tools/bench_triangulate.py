"""Time ut_triangulate_points (csrc/triangulate.hip) with device events: 512, 2048 and 8192 hands x 21 landmarks of the
recording's label poses, from 2 views (the two cameras of the frame that see the hand) and from 4 views (four ring cameras
with the recording's intrinsics around the hand, all seeing it), from exact windows and from windows with 1 px Gaussian
noise.  Prints one JSON line per case: microseconds per launch (median of --repeats windows), points per second, and the
mean and largest iteration count - counted by the float64 restatement of tests/triangulate_cases.py on the first 738 hands of
the case (it takes the same decisions; the kernel reports a status, not a count).  A new capability has no earlier time to
compare with, so two yardsticks stand beside each row:
  project_floor_us  ut_project_points on the same points and views x (mean iterations + 1): the start and every iteration
                    evaluate the forward projection once, so no solver built on that arithmetic can be faster
  and, once per view count, the float64 numpy restatement on 738 hands (host clock): the CPU baseline.

    python tools/bench_triangulate.py [--iters 50] [--repeats 7]
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
import triangulate_cases as tc  # noqa: E402
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


def label_scene(views):
    """The 738 label hands: landmarks [738,21,3] float64, table [R,32], cam_rows [738,views]."""
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    ja, xf, hand = mc.label_poses(lab)
    pts = fc.forward(hm, ja, fc.effective_wrist(xf, hand, 1.0, np.float64))
    if views == 2:          # the two cameras of the frame that see every landmark of the hand
        c = pipeline.label_candidates(lab, np.arange(lab["joint_angles"].shape[0]))
        table = c["cam_params"]
        frame = np.arange(738) // 2
        rows4 = frame[:, None] * 4 + np.arange(4)[None]
        win, ez = tc.project(table[rows4][:, :, None], pts[:, None], tc.FISHEYE62)
        wid, hgt = c["src_wh"]
        seen = ((ez > 0) & (win >= 0).all(-1) & (win[..., 0] < wid) & (win[..., 1] < hgt)).all(-1)
        assert np.all(seen.sum(1) == 2)
        rows = np.stack([rows4[i, seen[i]] for i in range(738)]).astype(np.int32)
    else:                   # four ring cameras around the middle of the hand
        table = np.concatenate([tc.ring_cameras(4, pts[i].mean(0), seed=i) for i in range(738)])
        rows = np.arange(738 * 4, dtype=np.int32).reshape(738, 4)
    return pts, table, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    ap.add_argument("--no-cpu", action="store_true", help="leave the numpy baseline out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulate.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    for views in (2, 4):
        pts738, table_np, rows738 = label_scene(views)
        table = torch.from_numpy(table_np).to(dev)
        for n in (512, 2048, 8192):
            idx = np.arange(n) % 738
            rows_np = rows738[idx]
            exact = tc.project(table_np[rows_np][:, :, None], pts738[idx][:, None], tc.FISHEYE62)[0]
            rows = torch.from_numpy(rows_np).to(dev)
            pts32 = torch.from_numpy(pts738[idx]).float().to(dev)
            proj_out = (torch.empty(n, views, 21, 2, dtype=torch.float64, device=dev), torch.empty(n, views, 21, dtype=torch.float64, device=dev),
                        torch.empty(n, views, 21, dtype=torch.uint8, device=dev))
            proj_us, _lo, _hi = timed(lambda: _native.project_points(pts32, rows, table, 636, 480, out=proj_out), args.iters, args.repeats)
            out = (torch.empty(n, 21, 3, dtype=torch.float64, device=dev), torch.empty(n, 21, 4, device=dev), torch.empty(n, views, 21, device=dev))
            for noise in (0.0, 1.0):
                win_np = exact + noise * rng.standard_normal(exact.shape)
                win = torch.from_numpy(win_np).to(dev)
                us, lo, hi = timed(lambda: _native.triangulate_points(win, rows, table, out=out), args.iters, args.repeats)
                m = min(n, 738)
                t0 = time.perf_counter()
                want = tc.triangulate(win_np[:m], rows_np[:m], table_np)
                dt = time.perf_counter() - t0
                info = out[1].cpu().numpy()
                its = want[3]
                err = float(np.linalg.norm(out[0].cpu().numpy()[:m] - want[0], axis=-1).max())
                print(json.dumps({"bench": "triangulate_points", "hands": n, "points": n * 21, "views": views, "noise_px": noise,
                                  "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                                  "points_per_s": round(n * 21 / (us * 1e-6)), "mean_iterations": round(float(its.mean()), 2),
                                  "max_iterations": int(its.max()),
                                  "converged_fraction": round(float((info[..., 3].astype(int) & _native.TRI_CONVERGED).astype(bool).mean()), 4),
                                  "vs_restatement_mm": err, "project_us_per_launch": round(proj_us, 2),
                                  "project_floor_us": round(proj_us * (float(its.mean()) + 1), 1),
                                  "times_the_project_floor": round(us / (proj_us * (float(its.mean()) + 1)), 1)}), flush=True)
                if not args.no_cpu and n == 512:
                    print(json.dumps({"bench": "triangulate_numpy_float64", "hands": m, "points": m * 21, "views": views, "noise_px": noise,
                                      "seconds": round(dt, 3), "points_per_s": round(m * 21 / dt)}), flush=True)


if __name__ == "__main__":
    main()
