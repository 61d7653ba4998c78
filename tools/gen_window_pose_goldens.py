#!/usr/bin/env python3
"""Golden vectors of the label-free crop placement (TEST INFRASTRUCTURE ONLY; runs where the reference checkout is
available - never on the GPU box).

    python tools/gen_window_pose_goldens.py [--ref /path/to/reference]

Runs the REFERENCE's own HandTracker.gen_crop_cameras_from_stereo_camera_with_window_hand_pose
(lib/tracker/tracker.py:111-219) and writes tests/golden/window_pose_rec00.npz.  lib.tracker.tracker imports cv2 and
(through lib.common.hand_skinning) pytorch3d at module level; the method itself uses neither, so import-only
placeholders are installed for them: `cv2` (INTER_LINEAR, read as a default argument value), `pytorch3d` and
`pytorch3d.transforms` (so3_exp_map = None).  The constructor gets a stub model with .to() and
getInputImageSizes() -> (96, 96).

Cases (recording_00 of the reference's sample data):
  realistic   frames 0, 20, .., 360, camera pairs (0, 1), (2, 3) and (1, 2) (cameras 1 and 2 are the ones that see the
              hands in this recording, so only the last pair has hands seen twice).  Keypoints: the label landmarks (the pinned FK
              of oracle.ref_camera) through the reference's world_to_eye / eye_to_window, plus seeded N(0, 2 px)
              noise, rounded to float32 like a 2-D detector's output.  A hand is in a view's dict when all 21
              landmarks are in front of the camera and >= 19 lie in the image.  Dict insertion order alternates
              between (0, 1) and (1, 0); every 7th case with hands in both dicts drops the first hand from the left
              dict, so that it is seen on the right only.
  adversarial keypoints at opposite image corners (10 + 11 of them), then 50 .. 200 px beyond them, and spread on
              the diagonal between the same corners (the fixed point diverges there; the reference raises or not
              as its arithmetic happens to go), and a zero-distortion
              Fisheye62 camera (f = 100, c = (320, 240)) with keypoints on c +- (100 r, 0): the reference raises for
              r >= 1.5 and not for r = 1.4.

Stored as flat tables.  Cases (the first n_real are the realistic ones, with their frame and pair): cams [N,2,14]
(ImageSizeX, ImageSizeY, fx, fy, cx, cy, k1..k6), c2w [N,2,4,4], raises [N].  Input keypoints, per case the left
dict's then the right dict's entries in insertion order: kp [M,21,2], kp_case, kp_view (0 left, 1 right), kp_hand.
Crop cameras of the cases that do not raise, in the result's hand order and then view-key order: crop_case,
crop_hand, crop_view, crop_f [P,2], crop_c [P,2], crop_T [P,4,4].
"""
import argparse
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from oracle import ref_camera  # noqa: E402

HM_FIELDS = ("joint_rotation_axes", "joint_rest_positions", "landmark_rest_positions",
             "landmark_rest_bone_weights", "landmark_rest_bone_indices", "joint_limits")
CAM_FIELDS = ("ImageSizeX", "ImageSizeY", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "k5", "k6")
OUT = os.path.join(REPO, "tests", "golden", "window_pose_rec00.npz")


def reference_tracker(ref: str):
    """The reference's HandTracker, imported from `ref` with import-only placeholders for cv2 / pytorch3d."""
    sys.path[:] = [ref] + [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    for m in [m for m in sys.modules if m == "lib" or m.startswith("lib.")]:
        del sys.modules[m]
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1
    p3d = types.ModuleType("pytorch3d")
    p3d_t = types.ModuleType("pytorch3d.transforms")
    p3d_t.so3_exp_map = None
    p3d.transforms = p3d_t
    sys.modules.update({"cv2": cv2, "pytorch3d": p3d, "pytorch3d.transforms": p3d_t})
    import lib.common.camera as rcam
    import lib.tracker.tracker as rtracker
    for mod in (rcam, rtracker):
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(ref)), mod.__file__
    method = rtracker.HandTracker.gen_crop_cameras_from_stereo_camera_with_window_hand_pose
    assert os.path.abspath(method.__code__.co_filename).startswith(os.path.abspath(ref))

    class StubModel:
        def to(self, device):
            return self

        def getInputImageSizes(self):
            return (96, 96)

    return rtracker.HandTracker(StubModel(), rtracker.HandTrackerOpts()), rcam


class Table:
    """Flat arrays (a few keys instead of one per value keeps the file small)."""

    def __init__(self):
        self.cases, self.kp, self.crops = [], [], []

    def run_case(self, tracker, cams, left, right):
        """cams: two reference camera models; left / right: {hand: [21,2]} in insertion order.  Returns the
        reference's result, or None where it raises "Unable to create crop camera"."""
        case = len(self.cases)
        for view, d in enumerate((left, right)):
            for h, kp in d.items():
                self.kp.append((case, view, h, kp))
        try:
            res = tracker.gen_crop_cameras_from_stereo_camera_with_window_hand_pose(
                camera_left=cams[0], camera_right=cams[1], window_hand_pose_left=left, window_hand_pose_right=right)
        except ValueError as e:
            assert e.args[0] == "Unable to create crop camera", e
            res = None
        self.cases.append((np.array([[c.width, c.height, *c.f, *c.c, *c.distort] for c in cams], np.float64),
                           np.stack([np.asarray(c.camera_to_world_xf, np.float64) for c in cams]), res is None))
        for h, per_hand in (res or {}).items():
            for v, cam in per_hand.items():
                self.crops.append((case, h, v, np.asarray(cam.f, np.float64), np.asarray(cam.c, np.float64),
                                   np.asarray(cam.camera_to_world_xf, np.float64)))
        return res

    def arrays(self):
        c, k, o = self.cases, self.kp, self.crops
        return {"cams": np.stack([x[0] for x in c]), "c2w": np.stack([x[1] for x in c]),
                "raises": np.array([x[2] for x in c]),
                "kp": np.stack([x[3] for x in k]), "kp_case": np.array([x[0] for x in k], np.int32),
                "kp_view": np.array([x[1] for x in k], np.int32), "kp_hand": np.array([x[2] for x in k], np.int64),
                "crop_case": np.array([x[0] for x in o], np.int32), "crop_hand": np.array([x[1] for x in o], np.int64),
                "crop_view": np.array([x[2] for x in o], np.int32), "crop_f": np.stack([x[3] for x in o]),
                "crop_c": np.stack([x[4] for x in o]), "crop_T": np.stack([x[5] for x in o])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("UMETRACK_REFERENCE",
                                                    os.path.join(os.path.dirname(REPO), "reference")),
                    help="checkout of the reference project (default: $UMETRACK_REFERENCE, else ../reference)")
    ref = ap.parse_args().ref
    labels = json.load(open(os.path.join(ref, "sample_data", "recording_00.json")))
    hm = {k: np.asarray(labels["hand_model"][k]) for k in HM_FIELDS}
    tracker, rcam = reference_tracker(ref)
    rng = np.random.default_rng(20261016)
    tab, frames, pairs = Table(), [], []
    stats = {"two_views": 0, "one_view": 0, "right_only": 0, "both_hands": 0, "order_10": 0}

    # ---- realistic set (keypoints as float32, like a 2-D detector's output)
    for fi in range(0, len(labels["joint_angles"]), 20):
        cams_all = [rcam.read_camera_from_json(cj).copy(
            camera_to_world_xf=np.asarray(labels["camera_to_world_transforms"][fi][ci], np.float64))
            for ci, cj in enumerate(labels["cameras"])]
        for pair in ((0, 1), (2, 3), (1, 2)):
            cams = [cams_all[pair[0]], cams_all[pair[1]]]
            order = (0, 1) if len(frames) % 2 == 0 else (1, 0)
            views = [{}, {}]
            for h in order:
                if labels["hand_confidences"][fi][h] < 0.5:
                    continue
                lm = ref_camera.landmarks_from_pose(hm, np.asarray(labels["joint_angles"][fi][h]),
                                                    np.asarray(labels["wrist_transforms"][fi][h]), h).astype(np.float64)
                for v, cam in enumerate(cams):
                    eye = cam.world_to_eye(lm)
                    win = cam.eye_to_window(eye)
                    inside = ((win[:, 0] >= 0) & (win[:, 0] <= cam.width - 1) & (win[:, 1] >= 0)
                              & (win[:, 1] <= cam.height - 1))
                    if (eye[:, 2] > 0).all() and inside.sum() >= 19:
                        views[v][h] = (win + rng.normal(0.0, 2.0, win.shape)).astype(np.float32)
            if len(frames) % 7 == 3 and views[0] and views[1]:
                del views[0][next(iter(views[0]))]
            if not views[0] and not views[1]:
                continue
            res = tab.run_case(tracker, cams, views[0], views[1])
            assert res is not None, f"realistic case of frame {fi} raised"
            frames.append(fi)
            pairs.append(pair)
            stats["two_views"] += sum(len(pv) == 2 for pv in res.values())
            stats["one_view"] += sum(len(pv) == 1 for pv in res.values())
            stats["right_only"] += sum(list(pv) == [1] for pv in res.values())
            stats["both_hands"] += len(res) == 2
            stats["order_10"] += list(res)[:2] == [1, 0]
    n_real = len(frames)

    # ---- adversarial set: a recording camera, keypoints at opposite corners of the image (10 + 11 of them) and
    # then up to 200 px beyond them, or spread along the diagonal between them
    cams = [rcam.read_camera_from_json(cj).copy(
        camera_to_world_xf=np.asarray(labels["camera_to_world_transforms"][0][ci], np.float64))
        for ci, cj in enumerate(labels["cameras"][:2])]
    w, ht = cams[0].width, cams[0].height
    t = np.linspace(0.0, 1.0, 21)[:, None]
    for off in (0, 50, 100, 150, 200):
        a, b = np.array([-off, -off], np.float64), np.array([w - 1 + off, ht - 1 + off], np.float64)
        a2, b2 = np.array([w - 1 + off, -off], np.float64), np.array([-off, ht - 1 + off], np.float64)
        corners = np.stack([a] * 10 + [b] * 11)
        corners2 = np.stack([a2] * 10 + [b2] * 11)
        for h in (0, 1):
            tab.run_case(tracker, cams, {h: corners}, {h: corners2})
            tab.run_case(tracker, cams, {h: a + t * (b - a)}, {})
    # ---- constructed raising case: zero-distortion Fisheye62, f = 100, c = (320, 240), keypoints on c +- (100 r, 0)
    zero = rcam.Fisheye62CameraModel(640, 480, (100.0, 100.0), (320.0, 240.0), [0.0] * 8, np.eye(4))
    for r in (1.0, 1.4, 1.5, 2.0):
        kp = np.stack([320.0 + 100.0 * r * np.linspace(-1.0, 1.0, 21), np.full(21, 240.0)], 1)
        for h in (0, 1):
            tab.run_case(tracker, [zero, zero], {h: kp}, {})

    out = tab.arrays()
    out["frame"], out["pair"], out["n_real"] = np.array(frames), np.array(pairs), np.array(n_real)
    np.savez_compressed(OUT, **out)
    raised = np.nonzero(out["raises"])[0].tolist()
    print(f"{OUT}: {n_real} realistic cases {stats}, {len(out['raises']) - n_real} adversarial (raise: {raised}), "
          f"{os.path.getsize(OUT)} bytes")
    assert all(v > 0 for v in stats.values()), stats
    assert not out["raises"][:n_real].any()


if __name__ == "__main__":
    main()
