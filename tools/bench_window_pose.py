"""Time the label-free crop placement (2-D keypoints -> crop cameras, lib/tracker/tracker.py:111-219) and the demo's
per-frame calls.
usage: python tools/bench_window_pose.py [--frames 1024] [--candidates 2048] [--calls 200]

Prints, as JSON lines:
  per_frame      median host-to-host latency of gen_crop_cameras_from_stereo_camera_with_window_hand_pose for a
                 two-hand stereo frame (cameras 1 and 2 of recording_00), kernel path and host path
  track_frame    median latency of track_frame_analysis next to track_frame on the same frame and crop cameras
  kernel         ut_gen_crop_cameras_from_window_points for N candidates by hipEvents (the entry's index read-back
                 included)
  hot_path       HotPath throughput in hand-frames/s on a keypoint-driven batch next to the label-driven plan of the
                 same frames (fp32 convolutions)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from absolutetrack_amd import _native, pipeline, synth  # noqa: E402
from absolutetrack_amd import tracker as tk  # noqa: E402
from oracle import ref_camera  # noqa: E402

DEV = "cuda:0"
PAIR = (1, 2)


def keypoints(lab, hm_np, fi, cams, rng):
    """{hand: [21,2]} per view of PAIR: projected label landmarks + N(0, 2 px), hands seen with >= 19 inside."""
    d = [{}, {}]
    for h in (0, 1):
        lm = ref_camera.landmarks_from_pose(hm_np, lab["joint_angles"][fi, h], lab["wrist_transforms"][fi, h],
                                            h).astype(np.float64)
        for v, ci in enumerate(PAIR):
            eye = cams[ci].world_to_eye(lm)
            win = cams[ci].eye_to_window(eye)
            inside = ((win[:, 0] >= 0) & (win[:, 0] <= cams[ci].width - 1) & (win[:, 1] >= 0)
                      & (win[:, 1] <= cams[ci].height - 1))
            if lab["hand_confidences"][fi, h] >= 0.5 and (eye[:, 2] > 0).all() and inside.sum() >= 19:
                d[v][h] = (win + rng.normal(0.0, 2.0, win.shape)).astype(np.float32)
    return d


def median_ms(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    lab = pipeline.load_labels()
    hm = pipeline.hand_model_from_labels(lab)
    hm_np = {k[3:]: v for k, v in lab.items() if k.startswith("hm.")}
    n_lab = lab["joint_angles"].shape[0]
    rng = np.random.default_rng(0)
    sd = synth.synthetic_state_dict(0)

    # ---- per-frame crop cameras: kernel path vs host path
    from lib.models.umetrack_model import UmeTrackModel
    from lib.tracker.tracker import HandTracker, HandTrackerOpts, InputFrame, ViewData
    fi = 200
    cams = pipeline.cameras_for_frame(lab, fi)
    left, right = keypoints(lab, hm_np, fi, cams, rng)
    assert sorted(left) == sorted(right) == [0, 1], "frame 200 should show both hands in both cameras"
    trk = HandTracker(UmeTrackModel(sd), HandTrackerOpts())
    call = lambda: trk.gen_crop_cameras_from_stereo_camera_with_window_hand_pose(cams[PAIR[0]], cams[PAIR[1]], left, right)
    host = lambda: tk.gen_crop_cameras_from_window_points(cams[PAIR[0]], cams[PAIR[1]], left, right, trk._input_size,
                                                          trk._hand_ratio_in_crop)
    for _ in range(10):
        call(), host()
    print(json.dumps({"per_frame": {"kernel_path_ms": round(median_ms(call, args.calls), 4),
                                    "host_path_ms": round(median_ms(host, args.calls), 4), "calls": args.calls}}))

    # ---- track_frame_analysis vs track_frame
    imgs = synth.synthetic_frames(1, seed=3)[0]
    sample = InputFrame(views=[ViewData(image=imgs[PAIR[0]], camera=cams[PAIR[0]], camera_angle=0),
                               ViewData(image=imgs[PAIR[1]], camera=cams[PAIR[1]], camera_angle=0)])
    cc = call()
    for _ in range(10):
        trk.track_frame_analysis(sample, hm, cc, None)
    a = median_ms(lambda: trk.track_frame_analysis(sample, hm, cc, None), args.calls)
    b = median_ms(lambda: trk.track_frame(sample, hm, cc), args.calls)
    print(json.dumps({"track_frame": {"track_frame_analysis_ms": round(a, 4), "track_frame_ms": round(b, 4)}}))

    # ---- kernel time for N candidates
    frame_ids = list(range(args.frames))
    per_label = {}                                      # label frames repeat with period n_lab: keypoints once each
    kps, rows, hands = [], [], []
    for fo, f in enumerate(frame_ids):
        lf = f % n_lab
        if lf not in per_label:
            per_label[lf] = keypoints(lab, hm_np, lf, pipeline.cameras_for_frame(lab, lf), rng)
        d = per_label[lf]
        for h in list(d[0]) + [h for h in d[1] if h not in d[0]]:
            kp = np.zeros((2, 21, 2))
            rr = [-1, -1]
            for v in range(2):
                if h in d[v]:
                    kp[v] = d[v][h]
                    rr[v] = fo * 4 + PAIR[v]
            kps.append(kp)
            rows.append(rr)
            hands.append(h)
    cam_params = pipeline.label_candidates(lab, frame_ids)["cam_params"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    n = args.candidates
    reps = (n + len(hands) - 1) // len(hands)
    kp_d = t(np.concatenate([np.stack(kps)] * reps)[:n])
    row_d = t(np.concatenate([np.asarray(rows, np.int32)] * reps)[:n])
    hand_d = t(np.concatenate([np.asarray(hands, np.int64)] * reps)[:n])
    cam_d = t(cam_params)
    gen = lambda: _native.gen_crop_cameras_from_window_points(cam_d, kp_d, row_d, hand_d, check_indices=False)
    for _ in range(3):
        gen()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        gen()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"kernel": {"candidates": n, "ms_per_call": round(e0.elapsed_time(e1) / 20, 4)}}))

    # ---- HotPath throughput: keypoint-driven plan vs label-driven plan of the same frames
    eng = _native.HipEngine(sd, DEV)
    try:
        src = torch.randint(0, 256, (args.frames * 4, 480, 636), dtype=torch.uint8, device=DEV,
                            generator=torch.Generator(device=DEV).manual_seed(1234))
        out = {}
        plans = {"keypoints": pipeline.crop_plan_from_window_points(cam_params, np.stack(kps), np.asarray(rows, np.int32),
                                                                    np.asarray(hands, np.int64), DEV),
                 "labels": pipeline.crop_plan_on_device(lab, hm, frame_ids, DEV)}
        for name, plan in plans.items():
            batch = pipeline.make_batch({k: v.cpu().numpy() for k, v in plan.items()}, src, DEV)
            hot = pipeline.HotPath(eng, hm, known_skeleton=True)
            for _ in range(2):
                hot.step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                hot.step(batch)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 5
            hot.check()
            out[name] = {"hand_frames": batch.n_samples, "crops": batch.n_crops,
                         "hand_frames_per_s": round(batch.n_samples / dt, 1)}
        print(json.dumps({"hot_path": out}))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
