"""Label-free crop placement from 2-D keypoints (lib/tracker/tracker.py:111-219, the reference's live demo path) on the
host: the drop-in HandTracker's call surface, and the host path against the goldens the reference's own method wrote
(tests/golden/window_pose_rec00.npz, tools/gen_window_pose_goldens.py).  No GPU needed."""
import inspect

import numpy as np
import pytest

from absolutetrack_amd import tracker as tk
from window_pose_cases import load_cases


class _StubModel:
    def to(self, device):
        return self

    def getInputImageSizes(self):
        return (96, 96)


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


def test_drop_in_tracker_has_the_demo_methods_with_the_reference_parameters():
    from lib.tracker.tracker import HandTracker
    sig = inspect.signature(HandTracker.gen_crop_cameras_from_stereo_camera_with_window_hand_pose)
    assert list(sig.parameters) == ["self", "camera_left", "camera_right", "window_hand_pose_left",
                                    "window_hand_pose_right"]
    sig = inspect.signature(HandTracker.track_frame_analysis)
    assert list(sig.parameters) == ["self", "sample", "hand_model", "crop_cameras", "gt_tracking"]


def _host(case):
    return tk.gen_crop_cameras_from_window_points(case["cams"][0], case["cams"][1], case["left"], case["right"],
                                                  np.array([96, 96]), 0.8)


def test_host_path_reproduces_the_reference_cameras(cases):
    real = [c for c in cases if c["real"]]
    assert len(real) > 50 and sum(len(pv) == 2 for c in real for pv in c["expected"].values()) > 10
    for case in real:
        got = _host(case)
        assert list(got) == list(case["expected"])
        for h, per_hand in case["expected"].items():
            assert list(got[h]) == list(per_hand)
            for v, (f, c, T) in per_hand.items():
                cam = got[h][v]
                np.testing.assert_allclose(cam.f, f, rtol=1e-12, atol=0)
                np.testing.assert_allclose(cam.c, c, rtol=1e-12, atol=0)
                np.testing.assert_allclose(cam.camera_to_world_xf, T, rtol=1e-12, atol=1e-12)
                assert (cam.width, cam.height) == (96, 96)


def test_host_path_raises_exactly_where_the_reference_raises(cases):
    adv = [c for c in cases if not c["real"]]
    assert any(c["raises"] for c in adv) and not all(c["raises"] for c in adv)
    for case in cases:
        if case["raises"]:
            with pytest.raises(ValueError, match="Unable to create crop camera"):
                _host(case)
        else:
            assert list(_host(case)) == list(case["expected"])


def test_tracker_without_a_device_runs_the_host_path(cases):
    from lib.tracker.tracker import HandTracker, HandTrackerOpts
    trk = HandTracker(_StubModel(), HandTrackerOpts())
    trk._device = "cpu"
    for case in cases[:6]:
        got = trk.gen_crop_cameras_from_stereo_camera_with_window_hand_pose(
            camera_left=case["cams"][0], camera_right=case["cams"][1], window_hand_pose_left=case["left"],
            window_hand_pose_right=case["right"])
        want = _host(case)
        assert list(got) == list(want) and all(list(got[h]) == list(want[h]) for h in want)
        for h in want:
            for v in want[h]:
                assert np.array_equal(got[h][v].camera_to_world_xf, want[h][v].camera_to_world_xf)
    # extra columns (e.g. a detector's z) are ignored, as in the reference's window_hand_pose[:, :2]
    case = cases[0]
    wide = {h: np.concatenate([kp, np.ones((21, 1), kp.dtype)], 1) for h, kp in case["left"].items()}
    got = trk.gen_crop_cameras_from_stereo_camera_with_window_hand_pose(case["cams"][0], case["cams"][1], wide,
                                                                         case["right"])
    want = _host(case)
    assert all(np.array_equal(got[h][v].f, want[h][v].f) for h in want for v in want[h])


def test_track_frame_analysis_without_hands_resets_history():
    from lib.tracker.tracker import HandTracker, HandTrackerOpts
    trk = HandTracker(_StubModel(), HandTrackerOpts())
    trk._valid_tracking_history[:] = True
    res = trk.track_frame_analysis(None, None, {}, None)
    assert res.hand_poses == {} and not trk._valid_tracking_history.any()
