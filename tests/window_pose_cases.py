"""Cases of tests/golden/window_pose_rec00.npz (written by tools/gen_window_pose_goldens.py from the reference's
HandTracker.gen_crop_cameras_from_stereo_camera_with_window_hand_pose) as drop-in cameras and keypoint dicts, and
keypoints of the label landmarks for frames the goldens do not hold."""
import os

import numpy as np

from absolutetrack_amd import geometry
from oracle import ref_camera


def load_cases(golden_dir):
    """[dict(real, cams (left, right), left {hand: kp}, right {hand: kp}, raises, expected {hand: {view: (f, c, T)}})]"""
    g = dict(np.load(os.path.join(golden_dir, "window_pose_rec00.npz")))
    cases = []
    for i in range(g["raises"].shape[0]):
        cams = []
        for v in range(2):
            p = g["cams"][i, v]
            cams.append(geometry.Fisheye62CameraModel(int(p[0]), int(p[1]), (p[2], p[3]), (p[4], p[5]), tuple(p[6:14]),
                                                      g["c2w"][i, v].copy()))
        views = [{}, {}]
        for j in np.nonzero(g["kp_case"] == i)[0]:
            views[int(g["kp_view"][j])][int(g["kp_hand"][j])] = g["kp"][j]
        expected = {}
        for j in np.nonzero(g["crop_case"] == i)[0]:
            expected.setdefault(int(g["crop_hand"][j]), {})[int(g["crop_view"][j])] = (
                g["crop_f"][j], g["crop_c"][j], g["crop_T"][j])
        cases.append({"real": i < int(g["n_real"]), "cams": cams, "left": views[0], "right": views[1],
                      "raises": bool(g["raises"][i]), "expected": expected})
    return cases


def label_keypoints(lab, hm_np, frame, hand, cam, rng, sigma=2.0):
    """Window keypoints [21,2] of a label hand in a drop-in camera (+ N(0, sigma) px noise), or None when the hand is
    not seen there: the generator's rule (all 21 landmarks in front of the camera, >= 19 inside the image)."""
    lm = ref_camera.landmarks_from_pose(hm_np, lab["joint_angles"][frame, hand], lab["wrist_transforms"][frame, hand],
                                        hand).astype(np.float64)
    eye = cam.world_to_eye(lm)
    win = cam.eye_to_window(eye)
    inside = (win[:, 0] >= 0) & (win[:, 0] <= cam.width - 1) & (win[:, 1] >= 0) & (win[:, 1] <= cam.height - 1)
    if lab["hand_confidences"][frame, hand] < 0.5 or not (eye[:, 2] > 0).all() or inside.sum() < 19:
        return None
    return (win + rng.normal(0.0, sigma, win.shape)).astype(np.float32)
