"""Time ut_fit_pose_views_scale (csrc/fit_views_scale.hip) with device events: --poses hands (default 8192) - the 74 hands of
tests/views_cases.py golden() repeated, their two seeing views, Fisheye62, exact windows of the label poses on the model x 1.1,
tracking starts +-0.05 rad on the 20 angles and the wrist's rotation / +-5 mm (tests/robust_cases.py tracking_starts, drawn per
copy, so that no two copies are the same problem) at scale 1 - under the squared loss and Huber at 3 px, free and fixed (fixed: at
1.1), and the three-launch calibration chain (free pass -> ut_pool_scale over groups of 74 -> fixed pass) end to end.  Prints one
JSON line per case: microseconds per launch (median of --repeats windows of --iters launches, and their spread), nanoseconds per
hand, mean and largest iteration count, microseconds per iteration, the fraction converged.

The yardstick is ut_fit_pose_views_robust (device code unchanged) with the same loss on the same windows and starts, on the model
x 1.1 - the problem the fixed pass solves.  Every round times one window of every case in a random order (seeded), each window
behind a lead-in of --lead launches of its own case that are not timed, so that a drift of the device's clock and whatever ran
before meet all cases alike; `over_views_fit` is the ratio of the medians per launch to the yardstick of the same loss,
`per_iteration_over_views_fit` of the times per iteration, and `yardstick_spread` the yardstick's own (max - min) / median, the
margin a ratio has to leave before it says anything.  No threshold is set.

    python tools/bench_views_scale.py [--poses 8192] [--iters 20] [--repeats 7] [--lead 2]
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

import robust_cases as rc  # noqa: E402
import scale_cases as sc  # noqa: E402
import views_cases as vc  # noqa: E402
from absolutetrack_amd import _native  # noqa: E402

SCALE = 1.1
GROUP = 74


def shuffled_rounds(fns, iters, repeats, lead, seed=0):
    """{name: (median, min, max) us per launch}: `repeats` rounds, each one timed window of every function in a random order,
    every window behind `lead` untimed launches of the same function."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rng = np.random.default_rng(seed)
    names = list(fns)
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for i in rng.permutation(len(names)):
            fn = fns[names[i]]
            for _ in range(lead):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[names[i]].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (float(np.median(t)), min(t), max(t)) for k, t in times.items()}


def blob_of(hm, dev):
    return torch.from_numpy(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"], hm["landmark_rest_positions"],
                                                    hm["landmark_rest_bone_weights"], hm["landmark_rest_bone_indices"])).reshape(-1, 321).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=8192, help="hands per launch, a multiple of 74 is not needed: the chain pools whole groups")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per case (the median is reported)")
    ap.add_argument("--lead", type=int, default=2, help="untimed launches in front of every timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_views_scale.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    g = vc.golden()
    n = args.poses
    idx = np.arange(n) % 74
    blob = blob_of(g["hm"], dev)
    blob_scaled = blob_of(sc.scaled_model(g["hm"], np.full(1, np.float32(SCALE)), np.float32), dev)
    two = vc.select(g, g["seeing"])
    truth = vc.posed(g, sc.scaled_model(g["hm"], np.full(74, SCALE)))
    window = vc.exact_windows(g["table"], two["cam_rows"], truth)
    table = torch.from_numpy(g["table"]).to(dev)
    win, rows, weights = (torch.from_numpy(a[idx]).to(dev) for a in (window, two["cam_rows"], two["weights"]))
    ja0, xf0 = rc.tracking_starts(dict(ja=g["ja"][idx], xf=g["xf"][idx]), 0)
    ja0, xf0 = torch.from_numpy(ja0).to(dev), torch.from_numpy(xf0).to(dev)
    mirror = torch.from_numpy(g["hand"][idx]).to(dev)
    fixed_at = torch.full((n,), SCALE, device=dev)
    n_chain = n - n % GROUP

    cases = [(f"views_{loss}", loss, None) for loss in ("squared", "huber")] + \
            [(f"{mode}_{loss}", loss, mode) for loss in ("squared", "huber") for mode in ("free", "fixed")]
    outs = {k: (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev)) for k, *_ in cases}
    infos = {k: torch.empty(n, 4 if mode is None else 6, device=dev) for k, _loss, mode in cases}
    scales = {k: torch.empty(n, device=dev) for k in outs}
    chain_buf = dict(ja=torch.empty(n_chain, 22, device=dev), xf=torch.empty(n_chain, 4, 4, device=dev), s=torch.empty(n_chain, device=dev),
                     info=torch.empty(n_chain, 6, device=dev), group=torch.empty(n_chain // GROUP, 4, device=dev),
                     ps=torch.empty(n_chain, device=dev), ja2=torch.empty(n_chain, 22, device=dev), xf2=torch.empty(n_chain, 4, 4, device=dev),
                     s2=torch.empty(n_chain, device=dev), info2=torch.empty(n_chain, 6, device=dev))

    def launch(k, loss, mode):
        if mode is None:
            return lambda: _native.fit_pose_views_robust(blob_scaled, win, rows, table, ja0, xf0, weights=weights, mirror=mirror, loss=loss,
                                                         loss_scale=rc.SCALE_PX, out=outs[k], info=infos[k])
        return lambda: _native.fit_pose_views_scale(blob, win, rows, table, ja0, xf0, weights=weights, mirror=mirror, loss=loss,
                                                    loss_scale=rc.SCALE_PX, init_scale=fixed_at if mode == "fixed" else None,
                                                    scale_mode=_native.UT_SCALE_FIXED if mode == "fixed" else _native.UT_SCALE_FREE,
                                                    out=outs[k], scale=scales[k], info=infos[k])

    def chain():
        b, m = chain_buf, slice(0, n_chain)
        _native.fit_pose_views_scale(blob, win[m], rows[m], table, ja0[m], xf0[m], weights=weights[m], mirror=mirror[m],
                                     out=(b["ja"], b["xf"]), scale=b["s"], info=b["info"])
        _native.pool_scale(b["s"], b["info"], GROUP, group=b["group"], pose_scale=b["ps"])
        _native.fit_pose_views_scale(blob, win[m], rows[m], table, b["ja"], b["xf"], weights=weights[m], mirror=mirror[m], init_scale=b["ps"],
                                     scale_mode=_native.UT_SCALE_FIXED, out=(b["ja2"], b["xf2"]), scale=b["s2"], info=b["info2"])

    fns = {k: launch(k, loss, mode) for k, loss, mode in cases}
    fns["chain_squared"] = chain
    t = shuffled_rounds(fns, args.iters, args.repeats, args.lead)
    result = {}
    for k, loss, mode in cases:
        us, lo, hi = t[k]
        r = infos[k].cpu().numpy()
        name = f"fit_pose_views_robust_{loss}" if mode is None else f"fit_pose_views_scale_{mode}_{loss}"
        result[k] = {"bench": name, "poses": n, "us_per_launch": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                     "ns_per_hand": round(us * 1e3 / n, 1), "mean_iterations": round(float(r[:, 2].mean()), 2),
                     "max_iterations": int(r[:, 2].max()), "us_per_iteration": round(us / float(r[:, 2].mean()), 2),
                     "converged_fraction": round(float((r[:, 3].astype(int) & 1).astype(bool).mean()), 4)}
        if mode is None:
            result[k]["yardstick_spread"] = round((hi - lo) / us, 4)
        else:
            s = scales[k].cpu().numpy().astype(np.float64)
            result[k]["worst_scale_error"] = float(np.abs(s - SCALE).max())
    for k, loss, mode in cases:
        if mode is not None:
            y = result[f"views_{loss}"]
            result[k]["over_views_fit"] = round(result[k]["us_per_launch"] / y["us_per_launch"], 3)
            result[k]["per_iteration_over_views_fit"] = round(result[k]["us_per_iteration"] / y["us_per_iteration"], 3)
    us, lo, hi = t["chain_squared"]
    r1, r2 = chain_buf["info"].cpu().numpy(), chain_buf["info2"].cpu().numpy()
    pooled = chain_buf["group"][:, 0].cpu().numpy().astype(np.float64)
    result["chain_squared"] = {"bench": "calibration_chain_free_pool_fixed_squared", "poses": n_chain, "groups": n_chain // GROUP,
                               "us_per_chain": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                               "ns_per_hand": round(us * 1e3 / n_chain, 1),
                               "mean_iterations_free": round(float(r1[:, 2].mean()), 2), "mean_iterations_fixed": round(float(r2[:, 2].mean()), 2),
                               "over_views_fit": round(us / result["views_squared"]["us_per_launch"] * n / n_chain, 3),
                               "worst_pooled_scale_error": float(np.abs(pooled - SCALE).max())}
    for row in result.values():
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
