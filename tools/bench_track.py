"""Time ut_track_pose_views (csrc/track_views.hip) with device events on two workloads, against what it replaces and against its
floor.  The detections are recording_00's: both hands' label poses through the two cameras that see most of the hand, 0.5 px noise
(tests/smooth_cases.py recording), every sequence started at its first frame's label, the cold results from the existing cold chain.

  2 x 369   one recording.  `track`: the one launch.  `loop_device`: the parent's loop as a device-only queue - 369 launches of
            ut_fit_pose_views with n = 2, frame t started from frame t - 1's output rows, no read-back and no decision.  `one_sequence`:
            the one launch on hand 1 alone; its time over 369 is the latency per frame a live caller sees, one wave's dependent work.
            Then host to host (wall clock, synchronised): tracker.track_hand_poses_in_views on hand 1 as it is now against the copy of
            its former per-frame loop, which tests/track_cases.py keeps.
  4096 x 16 sliding windows over the two hands.  `track` against `fit`: ONE ut_fit_pose_views launch over the same 65536 poses, every
            pose from the start the tracker gave it (the previous frame's tracked pose).  That launch is a floor: its poses are
            independent, the tracker's 16 frames of a sequence are not.

The timed windows of a workload's launches are interleaved - one window of each in turn, after five warm-ups each - so that a
drift of the device's clock meets all of them alike.  Prints one JSON line per measurement.  No threshold is set.

    python tools/bench_track.py [--iters 5] [--repeats 5] [--host-repeats 3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import smooth_cases as sm  # noqa: E402
import start_cases as sc  # noqa: E402
import track_cases as tk  # noqa: E402
import step_cases as st  # noqa: E402
from absolutetrack_amd import _native, hand, pipeline, tracker  # noqa: E402
from bench_views import interleaved  # noqa: E402

FRAMES = 369


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="launches (or queues of 369 launches) per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case (the median is reported)")
    ap.add_argument("--host-repeats", type=int, default=3, help="host-to-host calls of each tracker function")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track.py needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    put = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)
    recs = [sm.recording(0, FRAMES - 1, h, 2, 0.5) for h in (0, 1)]
    case = [r["views_case"] for r in recs]
    hm = case[0]["hm"]
    blob = put(_native.hand_model_blob(*(hm[k] for k in st.FIELDS))).reshape(1, 321)
    table = put(case[0]["table"], torch.float64)
    bank, seeds = put(sc.bank()), put(sc.seeds(), torch.float64)

    def gather(hands, frames):
        """Rows (hand, frame) of the two recordings on the device: window, cam_rows, weights, mirror."""
        pick = lambda f: np.stack([case[h][f][t] for h, t in zip(hands.reshape(-1), frames.reshape(-1))])
        return put(pick("window"), torch.float64), put(pick("cam_rows"), torch.int32), put(pick("weights")), put(hands.reshape(-1), torch.int64)

    def workload(hands, first, n_frames):
        """Sequences s = frames first[s] .. first[s] + n_frames - 1 of hand hands[s]: inputs, label starts, cold results, buffers."""
        n_seq = len(hands)
        frames = first[:, None] + np.arange(n_frames)[None]
        win, rows, w, mirror = gather(np.repeat(hands[:, None], n_frames, 1), frames)
        init = (put(np.stack([recs[h]["truth_ja"][f] for h, f in zip(hands, first)])), put(np.stack([recs[h]["truth_xf"][f] for h, f in zip(hands, first)])))
        cold = hand._cold_chain(blob, (win, rows, table), w, None, mirror, bank, seeds, sc.ITERS, 32, "squared", 3.0)
        n = n_seq * n_frames
        out = (torch.empty(n, 22, device=dev), torch.empty(n, 4, 4, device=dev))
        info, chosen = torch.empty(n, 4, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        track = lambda: _native.track_pose_views(blob, win, rows, table, n_frames, init[0], init[1], cold, w, None, mirror, out=out, info=info, chosen=chosen)
        return dict(win=win, rows=rows, w=w, mirror=mirror, init=init, cold=cold, out=out, info=info, chosen=chosen, track=track, n_seq=n_seq, n_frames=n_frames)

    def report(name, n_seq, n_frames, t, **more):
        us, lo, hi = t
        print(json.dumps(dict({"bench": name, "sequences": n_seq, "frames": n_frames, "us": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1)},
                              **more)), flush=True)

    # ------------------------------------------------------------------ 2 x 369
    both = workload(np.array([0, 1]), np.array([0, 0]), FRAMES)
    one = workload(np.array([1]), np.array([0]), FRAMES)
    fm = lambda t, tail: t.reshape((2, FRAMES) + tail).transpose(0, 1).contiguous()      # frame-major: what a per-frame loop launches on
    win_f, rows_f, w_f, mirror_f = fm(both["win"], (2, 21, 2)), fm(both["rows"], (2,)), fm(both["w"], (2, 21)), fm(both["mirror"], ())
    ja_f, xf_f, info_f = torch.empty(FRAMES, 2, 22, device=dev), torch.empty(FRAMES, 2, 4, 4, device=dev), torch.empty(FRAMES, 2, 4, device=dev)

    def loop_device():
        prev = both["init"]
        for t in range(FRAMES):
            _native.fit_pose_views(blob, win_f[t], rows_f[t], table, prev[0], prev[1], weights=w_f[t], mirror=mirror_f[t], out=(ja_f[t], xf_f[t]), info=info_f[t])
            prev = (ja_f[t], xf_f[t])

    t = interleaved({"track": both["track"], "loop_device": loop_device, "one_sequence": one["track"]}, args.iters, args.repeats)
    taken = int((both["chosen"] == _native.UT_TRACK_COLD).sum())
    report("track_pose_views", 2, FRAMES, t["track"], over_loop_device=round(t["track"][0] / t["loop_device"][0], 4), cold_rows_taken=taken,
           mean_iterations=round(float(both["info"][:, 2].mean()), 2))
    report("fit_pose_views_loop_device_only", 2, FRAMES, t["loop_device"], launches=FRAMES)
    report("track_pose_views", 1, FRAMES, t["one_sequence"], us_per_frame=round(t["one_sequence"][0] / FRAMES, 2))

    # host to host: the tracker function as it is against its former loop
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    n_cam = lab["cameras"].shape[0]
    c1 = case[1]
    cams = [[pipeline.cameras_for_frame(lab, f)[int(r) % n_cam] for r in c1["cam_rows"][f]] for f in range(FRAMES)]
    label = tracker.SingleHandPose(recs[1]["truth_ja"][0], recs[1]["truth_xf"][0])
    calls = {"now": lambda: tracker.track_hand_poses_in_views(model, cams, c1["window"], 1, init=label, weights=c1["weights"]),
             "former_loop": lambda: tk.former_track_loop(model, cams, c1["window"], 1, label, tracker.RECOVER_RATIO, c1["weights"])}
    wall = {k: [] for k in calls}
    results = {}
    for k, fn in calls.items():
        results[k] = fn()                                 # warm-up, and the results to compare
    for _ in range(args.host_repeats):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(results["now"][1].view(np.uint32), results["former_loop"][1].view(np.uint32)) and np.array_equal(results["now"][2], results["former_loop"][2]))
    med = {k: float(np.median(v)) for k, v in wall.items()}
    print(json.dumps({"bench": "tracker.track_hand_poses_in_views host to host", "frames": FRAMES, "ms_now": round(med["now"], 1),
                      "ms_former_loop": round(med["former_loop"], 1), "now_over_former": round(med["now"] / med["former_loop"], 4),
                      "ms_now_all": [round(v, 1) for v in wall["now"]], "ms_former_all": [round(v, 1) for v in wall["former_loop"]],
                      "same_bits": same, "recovered_frames": int(results["now"][2].sum())}), flush=True)

    # ------------------------------------------------------------------ 4096 x 16
    n_seq, n_frames = 4096, 16
    s = np.arange(n_seq)
    big = workload(s % 2, (s // 2 * 5) % (FRAMES - n_frames), n_frames)
    big["track"]()
    torch.cuda.synchronize()
    # every pose's start as the tracker had it: the previous frame's tracked row, the sequence's init at frame 0
    ja = big["out"][0].reshape(n_seq, n_frames, 22)
    xf = big["out"][1].reshape(n_seq, n_frames, 4, 4)
    start_ja = torch.cat([big["init"][0][:, None], ja[:, :-1]], 1).reshape(-1, 22).contiguous()
    start_xf = torch.cat([big["init"][1][:, None], xf[:, :-1]], 1).reshape(-1, 4, 4).contiguous()
    fit_out, fit_info = (torch.empty(n_seq * n_frames, 22, device=dev), torch.empty(n_seq * n_frames, 4, 4, device=dev)), torch.empty(n_seq * n_frames, 4, device=dev)
    fit = lambda: _native.fit_pose_views(blob, big["win"], big["rows"], table, start_ja, start_xf, weights=big["w"], mirror=big["mirror"], out=fit_out, info=fit_info)
    t = interleaved({"track": big["track"], "fit": fit}, args.iters, args.repeats)
    warm = big["chosen"] == _native.UT_TRACK_WARM
    same = bool(torch.equal(fit_out[0][warm].view(torch.int32), big["out"][0][warm].view(torch.int32)))
    report("track_pose_views", n_seq, n_frames, t["track"], over_one_fit_launch=round(t["track"][0] / t["fit"][0], 4),
           cold_rows_taken=int((big["chosen"] == _native.UT_TRACK_COLD).sum()), warm_rows_equal_the_fit=same)
    report("fit_pose_views", n_seq * n_frames, 1, t["fit"], mean_iterations=round(float(fit_info[:, 2].mean()), 2))


if __name__ == "__main__":
    main()
