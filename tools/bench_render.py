"""Time ut_render_mesh (csrc/render.hip) on the recording's 788-vertex hand mesh with device events: 512, 2048 and 8192 poses
with 2 views each, all three outputs, next to ut_skin_mesh on the same poses in the same process.  Prints one JSON line per
case: microseconds per launch (median of the timed windows), the output bytes the launch writes (9216 x 9 B per crop) over
that time, and that rate as a fraction of the achievable HBM bandwidth (--hbm-tbs, default 6.3 TB/s).

    python tools/bench_render.py [--iters 100] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from absolutetrack_amd import _native, hand, pipeline  # noqa: E402


def timed(fn, iters, repeats):
    for _ in range(10):
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
    ap.add_argument("--iters", type=int, default=100, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per case (the median is reported)")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM bandwidth the rate is compared with, TB/s")
    ap.add_argument("--mesh", default=os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = np.load(args.mesh)
    lab = pipeline.load_labels()
    hm = pipeline.hand_model_from_labels(lab)._replace(mesh_vertices=torch.from_numpy(g["rec00.mesh_vertices"]),
                                                       mesh_triangles=torch.from_numpy(g["rec00.mesh_triangles"]),
                                                       dense_bone_weights=torch.from_numpy(g["rec00.dense_bone_weights"]))
    mesh, blob = hand.device_mesh(hm, dev), hand.device_blob(hm, dev)
    n_frames = lab["joint_angles"].shape[0]
    plan = pipeline.crop_plan_on_device(lab, hm, range(n_frames), dev)
    c = pipeline.label_candidates(lab, range(n_frames))
    two = torch.nonzero(plan["sample_range"][:, 1] - plan["sample_range"][:, 0] == 2).reshape(-1)
    ja_all = torch.from_numpy(c["joint_angles"]).to(dev)
    xf_all = torch.from_numpy(c["wrist_xf"]).to(dev)
    hand_all = torch.from_numpy(c["hand_idx"]).to(dev)
    for n in (512, 2048, 8192):
        idx = two[torch.arange(n, device=dev) % two.shape[0]]
        ja, xf, mirror = ja_all[idx].contiguous(), xf_all[idx].contiguous(), hand_all[idx].contiguous()
        first = plan["sample_range"][idx, 0]
        crop_params = torch.stack([plan["crop_params"][first], plan["crop_params"][first + 1]], 1).reshape(-1, 24).contiguous()
        ends = torch.arange(1, n + 1, device=dev) * 2
        sample_range = torch.stack([ends - 2, ends], 1)
        verts = torch.empty(n, mesh.n_vertices, 3, device=dev)
        depth = torch.empty(2 * n, 96, 96, device=dev)
        tri = torch.empty(2 * n, 96, 96, dtype=torch.int32, device=dev)
        shade = torch.empty(2 * n, 96, 96, dtype=torch.uint8, device=dev)
        us_skin = timed(lambda: _native.skin_mesh(mesh, blob, ja, xf, mirror=mirror, out=verts), args.iters, args.repeats)
        us, lo, hi = timed(lambda: _native.render_mesh(mesh, verts, crop_params, sample_range, depth=depth, tri=tri, shade=shade),
                           args.iters, args.repeats)
        covered = float((tri >= 0).float().mean())
        out_bytes = 2 * n * 9216 * 9
        tbs = out_bytes / (us * 1e-6) / 1e12
        print(json.dumps({"bench": "render_mesh", "poses": n, "crops": 2 * n, "vertices": mesh.n_vertices,
                          "triangles": mesh.n_triangles, "covered_fraction": round(covered, 3), "us_per_launch": round(us, 2),
                          "us_min": round(lo, 2), "us_max": round(hi, 2), "out_mbytes": round(out_bytes / 1e6, 2),
                          "out_tb_per_s": round(tbs, 3), "fraction_of_achievable_hbm": round(tbs / args.hbm_tbs, 3),
                          "crops_per_s": round(2 * n / (us * 1e-6)), "skin_mesh_us_per_launch": round(us_skin[0], 2)}), flush=True)


if __name__ == "__main__":
    main()
