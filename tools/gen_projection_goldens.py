#!/usr/bin/env python3
"""Golden vectors of the landmark projection (TEST INFRASTRUCTURE ONLY; runs where the reference checkout is available -
never on the GPU box).

    python tools/gen_projection_goldens.py [--ref /path/to/reference]

Runs the REFERENCE's own lib.common.camera (read_camera_from_json, world_to_eye, eye_to_window: lib/common/camera.py:76-94,
296-312 and the Fisheye62 evaluate) on recording_00 of its sample data and writes tests/golden/projection_rec00.npz.

Cases: frames 0, 10, .., 360 x the 4 cameras x both hands.  Points: the 21 label landmarks (the pinned FK of
oracle.ref_camera) rounded to float32 - the precision the kernels hold points in - and widened back before the
reference's functions see them.  Hands with confidence < 0.5 are kept out.

Stored: cams [4,14] (ImageSizeX, ImageSizeY, fx, fy, cx, cy, k1 k2 k3 k4 p1 p2 k5 k6), frame [F], c2w [F,4,4,4], hand [N],
case_frame [N] (index into frame), landmarks f32 [N,21,3], window f64 [N,4,21,2] = eye_to_window(world_to_eye(p)) per
camera, eye_z f64 [N,4,21] = world_to_eye(p)[..., 2]."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from oracle import ref_camera  # noqa: E402

HM_FIELDS = ("joint_rotation_axes", "joint_rest_positions", "landmark_rest_positions",
             "landmark_rest_bone_weights", "landmark_rest_bone_indices", "joint_limits")
CAM_FIELDS = ("ImageSizeX", "ImageSizeY", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "k5", "k6")
OUT = os.path.join(REPO, "tests", "golden", "projection_rec00.npz")


def reference_camera_module(ref: str):
    sys.path[:] = [ref] + [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    for m in [m for m in sys.modules if m == "lib" or m.startswith("lib.")]:
        del sys.modules[m]
    import lib.common.camera as rcam
    assert os.path.abspath(rcam.__file__).startswith(os.path.abspath(ref)), rcam.__file__
    return rcam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("UMETRACK_REFERENCE", os.path.join(os.path.dirname(REPO), "reference")),
                    help="checkout of the reference project (default: $UMETRACK_REFERENCE, else ../reference)")
    ref = ap.parse_args().ref
    labels = json.load(open(os.path.join(ref, "sample_data", "recording_00.json")))
    hm = {k: np.asarray(labels["hand_model"][k]) for k in HM_FIELDS}
    rcam = reference_camera_module(ref)
    frames = list(range(0, len(labels["joint_angles"]), 10))
    c2w = np.asarray([labels["camera_to_world_transforms"][f] for f in frames], np.float64)
    hands, case_frame, lms, wins, zs = [], [], [], [], []
    for k, fi in enumerate(frames):
        cams = [rcam.read_camera_from_json(cj).copy(camera_to_world_xf=c2w[k, ci]) for ci, cj in enumerate(labels["cameras"])]
        for h in (0, 1):
            if labels["hand_confidences"][fi][h] < 0.5:
                continue
            lm = ref_camera.landmarks_from_pose(hm, np.asarray(labels["joint_angles"][fi][h]),
                                                np.asarray(labels["wrist_transforms"][fi][h]), h).astype(np.float32)
            eye = [cam.world_to_eye(lm.astype(np.float64)) for cam in cams]
            hands.append(h)
            case_frame.append(k)
            lms.append(lm)
            wins.append(np.stack([cam.eye_to_window(e) for cam, e in zip(cams, eye)]))
            zs.append(np.stack([e[:, 2] for e in eye]))
    cam_rows = np.array([[cj[f] if f in cj else cj["Camera"][f] for f in CAM_FIELDS] for cj in labels["cameras"]], np.float64)
    out = {"cams": cam_rows, "frame": np.array(frames, np.int32), "c2w": c2w, "hand": np.array(hands, np.int64),
           "case_frame": np.array(case_frame, np.int32), "landmarks": np.stack(lms), "window": np.stack(wins).astype(np.float64),
           "eye_z": np.stack(zs).astype(np.float64)}
    assert out["window"].dtype == np.float64 and np.isfinite(out["window"]).all()
    np.savez_compressed(OUT, **out)
    inside = (out["window"] >= 0).all(-1) & (out["window"][..., 0] < cam_rows[0, 0]) & (out["window"][..., 1] < cam_rows[0, 1])
    print(f"{OUT}: {len(hands)} (frame, hand) cases x 4 cameras x 21 landmarks, {inside.mean():.2f} inside the image, "
          f"{(out['eye_z'] > 0).mean():.2f} in front, {os.path.getsize(OUT)} bytes")
    assert 0.1 < inside.mean() < 0.9 and (out["eye_z"] <= 0).any()


if __name__ == "__main__":
    main()
