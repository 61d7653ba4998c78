"""Per-frame tracker with the reference's call surface (lib/tracker/tracker.py:40-412,
lib/tracker/perspective_crop.py:19-180, lib/tracker/tracking_result.py:14-30).

Host code here is parameter plumbing only: crop-camera parameters (a few 4x4 products per hand),
packing of kernel argument rows, dict bookkeeping.  The heavy steps run natively:
  * forward kinematics of the crop points / landmarks  -> csrc/fk.hip    (ut_fk)
  * fisheye->pinhole resampling of every crop          -> csrc/warp.hip  (ut_warp_crops)
  * the network                                        -> ut_backbone + ut_fuse_temporal_regress
"""
import contextlib
import logging
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _native, geometry
from .geometry import CameraModel, PinholePlaneCameraModel
from .hand import NUM_HANDS, NUM_JOINTS_PER_HAND, RIGHT_HAND_INDEX, HandModel, scaled_hand_model, skin_landmarks, skin_mesh
from .hand import FIT_CONVERGED, fit_landmarks, fit_landmarks_info, fit_landmarks_views, fit_landmarks_views_cold, pose_uncertainty_views, smooth_poses
from .hand import RECOVER_FLOOR_PX, RECOVER_RATIO, TRACK_COLD, track_landmarks_views
from .hand import ScaleCalibration, calibrate_scale, calibrate_scale_in_views
from .hand import device_blob, fk_device, render_mesh as _render_mesh
from .model import InputFrameData, InputFrameDesc, InputSkeletonData, RegressorOutput

logger = logging.getLogger(__name__)

MM_TO_M = 0.001
M_TO_MM = 1000.0
MIN_OBSERVED_LANDMARKS = 21
CONFIDENCE_THRESHOLD = 0.5
MAX_VIEW_NUM = 2


# ----------------------------------------------------------------------------- tracking_result.py
class SingleHandPose(NamedTuple):
    """joint angles (one per DoF) + root-to-world wrist transform (mm)."""
    joint_angles: np.ndarray = np.zeros(NUM_JOINTS_PER_HAND, dtype=np.float32)
    wrist_xform: np.ndarray = np.eye(4, dtype=np.float32)
    hand_confidence: float = 1.0


class TrackingResult(NamedTuple):
    hand_poses: Dict[int, SingleHandPose] = {}
    num_views: Dict[int, int] = {}
    predicted_scales: Dict[int, float] = {}


# ----------------------------------------------------------------------------- perspective_crop.py
def neutral_joint_angles(up: HandModel, lower_factor: float = 0.5) -> torch.Tensor:
    lim = up.joint_limits
    assert lim is not None
    return lim[..., 0] * lower_factor + lim[..., 1] * (1 - lower_factor)


def skin_landmarks_np(hand_model: HandModel, joint_angles: np.ndarray, wrist_transforms: np.ndarray) -> np.ndarray:
    out = skin_landmarks(hand_model, torch.from_numpy(np.asarray(joint_angles)).float(),
                         torch.from_numpy(np.asarray(wrist_transforms)).float())
    return out.cpu().numpy()


def _left_handed(wrist_xform: np.ndarray, hand_idx: int) -> np.ndarray:
    xf = np.array(wrist_xform, copy=True)
    if hand_idx == RIGHT_HAND_INDEX:      # the hand model is a left hand: mirror x for right hands
        xf[:, 0] *= -1
    return xf


def _mirror_flag(hand_idx: int) -> torch.Tensor:
    """The `mirror` of one hand for the hand.py wrappers: 1 for the right hand."""
    return torch.tensor(1 if hand_idx == RIGHT_HAND_INDEX else 0)


def _start_tensors(pose: Optional[SingleHandPose]):
    """A pose as the `init` of the hand.py fits: (joint_angles, wrist_transforms) float32 tensors, None for None."""
    if pose is None:
        return None
    return torch.from_numpy(np.asarray(pose.joint_angles, np.float32)), torch.from_numpy(np.asarray(pose.wrist_xform, np.float32))


def _pose_from_fit(ja: torch.Tensor, xf: torch.Tensor, fit_info: torch.Tensor) -> SingleHandPose:
    """The pose a fit returned: hand_confidence is 1 when it converged, else 0."""
    return SingleHandPose(joint_angles=ja.numpy(), wrist_xform=xf.numpy(), hand_confidence=1.0 if int(fit_info[3]) & FIT_CONVERGED else 0.0)


def landmarks_from_hand_pose(hand_model: HandModel, hand_pose: SingleHandPose, hand_idx: int) -> np.ndarray:
    """World-space landmarks [21,3] of a pose (lib/tracker/perspective_crop.py:40-51)."""
    hit = _landmark_memo.get(hand_model, hand_idx, hand_pose.joint_angles, hand_pose.wrist_xform)
    if hit is not None:
        return hit
    return skin_landmarks_np(hand_model, hand_pose.joint_angles, _left_handed(hand_pose.wrist_xform, hand_idx))


def hand_pose_from_landmarks(hand_model: HandModel, landmarks: np.ndarray, hand_idx: int,
                             init: Optional[SingleHandPose] = None) -> SingleHandPose:
    """The pose whose world-space landmarks are `landmarks` [21,3] (mm): the inverse of landmarks_from_hand_pose, on the
    HIP kernel csrc/fit.hip (hand.fit_landmarks).  The result goes straight into landmarks_from_hand_pose,
    mesh_from_hand_pose, render_hand_pose and gen_crop_cameras: its wrist transform is the proper one, right hands are
    mirrored by those consumers.  init: a pose to start from (e.g. last frame's); None starts from the rest pose aligned to
    the landmarks.  hand_confidence is 1 when the fit converged and 0 when it stopped at its iteration limit or refused
    the landmarks (not finite)."""
    kp = torch.from_numpy(np.ascontiguousarray(landmarks, np.float32)).reshape(21, 3)
    return _pose_from_fit(*fit_landmarks(hand_model, kp, init=_start_tensors(init), mirror=_mirror_flag(hand_idx)))


def hand_poses_from_keypoints(hand_model: HandModel, keypoints: np.ndarray, valid: np.ndarray
                              ) -> List[Dict[int, SingleHandPose]]:
    """Poses for a whole sequence of keypoints in the layout of the eval result files: keypoints [n_hands, n_frames, 21, 3]
    (mm, world; hand 1 is the right hand), valid [n_hands, n_frames].  Returns one dict per frame, hand index ->
    SingleHandPose, holding the hands that are valid in that frame.
    A valid frame is warm-started from the latest earlier valid frame of the same hand and cold-started when there is
    none, so frame t is fitted after frame t - 1; the hands of a frame share one launch per kind of start.  A warm start can
    end in a local minimum when the hand moved far: a frame whose warm-started fit does not converge is fitted again from
    the cold start, and the better of the two (lower residual) is kept."""
    keypoints, valid = np.asarray(keypoints), np.asarray(valid, bool)
    n_hands, n_frames = valid.shape
    if keypoints.shape != (n_hands, n_frames, 21, 3):
        raise ValueError(f"keypoints must be [{n_hands},{n_frames},21,3], got {keypoints.shape}")
    dev = fk_device()
    kp = torch.from_numpy(np.ascontiguousarray(keypoints, np.float32)).to(dev)
    last: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
    out: List[Dict[int, SingleHandPose]] = []

    def fit(hands, warm: bool):
        start = (torch.stack([last[h][0] for h in hands]), torch.stack([last[h][1] for h in hands])) if warm else None
        mirror = torch.tensor([1 if h == RIGHT_HAND_INDEX else 0 for h in hands], device=dev)
        ja, xf, info = fit_landmarks(hand_model, kp[hands, t], init=start, mirror=mirror)
        return ja, xf, info.cpu().numpy()

    for t in range(n_frames):
        found: Dict[int, Tuple[torch.Tensor, torch.Tensor, np.ndarray]] = {}
        warm = [h for h in range(n_hands) if valid[h, t] and h in last]
        cold = [h for h in range(n_hands) if valid[h, t] and h not in last]
        if warm:
            ja, xf, info = fit(warm, True)
            for k, h in enumerate(warm):
                found[h] = (ja[k], xf[k], info[k])
                if not int(info[k, 3]) & FIT_CONVERGED:
                    cold.append(h)
        if cold:
            ja, xf, info = fit(cold, False)
            for k, h in enumerate(cold):
                if h not in found or info[k, 0] < found[h][2][0]:
                    found[h] = (ja[k], xf[k], info[k])
        poses = {}
        for h in sorted(found):
            ja, xf, info = found[h]
            last[h] = (ja, xf)
            poses[h] = SingleHandPose(joint_angles=ja.cpu().numpy(), wrist_xform=xf.cpu().numpy(),
                                      hand_confidence=1.0 if int(info[3]) & FIT_CONVERGED else 0.0)
        out.append(poses)
    return out


def mesh_from_hand_pose(hand_model: HandModel, hand_pose: SingleHandPose, hand_idx: int, normals: bool = False):
    """World-space mesh vertices [V,3] of a pose, or (vertices, unit normals) with normals=True: the mesh twin of
    landmarks_from_hand_pose.  The hand model is a left hand: right hands get column 0 of the wrist transform negated, on
    the device (the same values as _left_handed gives), so that the normals of both hands point outwards."""
    res = skin_mesh(hand_model, torch.from_numpy(np.asarray(hand_pose.joint_angles)).float(),
                    torch.from_numpy(np.asarray(hand_pose.wrist_xform)).float(), normals=normals, mirror=_mirror_flag(hand_idx))
    if normals:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy()


def render_hand_pose(hand_model: HandModel, hand_pose: SingleHandPose, hand_idx: int, crop_cameras):
    """The pose drawn into its crop cameras - the dict (or list) of PinholePlaneCameraModel that gen_crop_cameras returns for
    the hand, at most two: (depth [V,96,96] f32, tri [V,96,96] i32, shade [V,96,96] u8) as numpy arrays, in the cameras'
    order.  The companion of mesh_from_hand_pose; right hands are un-mirrored the same way, and their crop cameras are
    x-mirrored, so both hands come out as left hands like the crops the network reads."""
    cams = list(crop_cameras.values()) if isinstance(crop_cameras, dict) else list(crop_cameras)
    res = _render_mesh(hand_model, torch.from_numpy(np.asarray(hand_pose.joint_angles)).float()[None],
                       torch.from_numpy(np.asarray(hand_pose.wrist_xform)).float()[None], cams,
                       mirror=torch.tensor([1 if hand_idx == RIGHT_HAND_INDEX else 0]),
                       sample_range=torch.tensor([[0, len(cams)]]))
    return tuple(r.cpu().numpy() for r in res)


def project_landmarks(cameras: List[CameraModel], landmarks_world: np.ndarray) -> np.ndarray:
    """[n_cams,P,2] window coordinates of world points [P,3] in every camera: camera.eye_to_window(camera.world_to_eye(p))
    of the reference's analysis scripts (run_eval_known_skeleton_analysis.py:296-358), for all cameras in one
    ut_project_points launch when they are all Fisheye62 or all pinhole models without distortion; any other camera
    model goes through its own host methods, as gen_crop_cameras_from_window_points does."""
    pts = np.asarray(landmarks_world)
    kinds = {type(c) for c in cameras}
    native = len(cameras) > 0 and pts.ndim == 2 and (kinds == {geometry.Fisheye62CameraModel} or kinds == {PinholePlaneCameraModel})
    if native:                               # the kernel serves these cameras: no host fallback, a missing device is an error
        dev = fk_device()
        table = torch.from_numpy(np.stack([geometry.pack_camera_model(c) for c in cameras])).to(dev)
        rows = torch.arange(len(cameras), dtype=torch.int32, device=dev)[None]
        win, _, _ = _native.project_points(torch.from_numpy(np.ascontiguousarray(pts, np.float32))[None].to(dev), rows, table,
                                           int(cameras[0].width), int(cameras[0].height))
        return win[0].cpu().numpy()
    return project_landmarks_host(cameras, pts)


def project_landmarks_host(cameras: List[CameraModel], landmarks_world: np.ndarray) -> np.ndarray:
    """project_landmarks through the cameras' own numpy methods (float64), any camera model."""
    pts = np.asarray(landmarks_world, np.float64)
    return np.stack([cam.eye_to_window(cam.world_to_eye(pts)) for cam in cameras]) if len(cameras) else np.zeros((0,) + pts.shape[:-1] + (2,))


def _native_camera_table(cameras: List[CameraModel], who: str) -> np.ndarray:
    """The cameras as rows of one kernel table: all Fisheye62, or all pinhole without distortion.  ValueError names any other
    model (no host fallback)."""
    kinds = {type(c) for c in cameras}
    if len(cameras) == 0:
        raise ValueError(f"{who}: no cameras")
    if kinds != {geometry.Fisheye62CameraModel} and kinds != {PinholePlaneCameraModel}:
        raise ValueError(f"{who}: cameras must all be Fisheye62CameraModel or all be PinholePlaneCameraModel, got "
                         + ", ".join(sorted(k.__name__ for k in kinds)))
    for c in cameras:
        if isinstance(c, PinholePlaneCameraModel) and len(tuple(c.distort)) > 0:
            raise ValueError(f"{who}: a PinholePlaneCameraModel with distortion coefficients is not served")
    return np.stack([geometry.pack_camera_model(c) for c in cameras])


def _window_inputs(who: str, cameras: List[CameraModel], window, weights, shape, name: str = "window_keypoints"):
    """What the functions on detections in the cameras check alike: (the cameras' kernel table, `window` as a contiguous float64
    array of `shape` - a dimension given by its name is free -, weights as float32 with the window's dims but the last, or None).
    `name` is how the caller's message calls the window."""
    table = _native_camera_table(cameras, who)
    win = np.ascontiguousarray(window, np.float64)
    if win.ndim != len(shape) or any(not isinstance(e, str) and e != d for e, d in zip(shape, win.shape)):
        raise ValueError(f"{name} must be [{','.join(map(str, shape))}], got {win.shape}")
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float32)
        if weights.shape != win.shape[:-1]:
            raise ValueError(f"weights must be {win.shape[:-1]}, got {weights.shape}")
    return table, win, weights


def triangulate_landmarks(cameras: List[CameraModel], window: np.ndarray, weights: Optional[np.ndarray] = None,
                          with_information: bool = False):
    """The inverse of project_landmarks: window coordinates [n_cams,P,2] of P points in every camera -> (world points [P,3]
    float64, info [P,4] float32: rms reprojection residual px, sigma - mm per px of detection noise -, views used, status
    bits _native.TRI_*), one ut_triangulate_points launch (csrc/triangulate.hip).  weights [n_cams,P] >= 0: how much each
    detection counts, 0 where the camera does not see the point (the window there is not read); None = all 1.  The cameras
    must all be Fisheye62 or all be pinhole models without distortion: any other model raises ValueError naming it - there
    is no host implementation.  with_information=True: one ut_triangulate_points_info launch instead, and a third result,
    sqrt_info [P,6] float32 - the lower Cholesky factor (l00, l10, l11, l20, l21, l22) of each point's 3 x 3 information
    matrix, px per mm, all 0 where the point carries none: what hand.fit_landmarks_info reads."""
    table, win, weights = _window_inputs("triangulate_landmarks", cameras, window, weights, (len(cameras), "P", 2), "window")
    dev = fk_device()
    rows = torch.arange(len(cameras), dtype=torch.int32, device=dev)[None]
    entry = _native.triangulate_points_info if with_information else _native.triangulate_points
    out = entry(torch.from_numpy(win)[None].to(dev), rows, torch.from_numpy(table).to(dev),
                weights=None if weights is None else torch.from_numpy(weights)[None].to(dev))
    if with_information:
        return out[0][0].cpu().numpy(), out[1][0].cpu().numpy(), out[3][0].cpu().numpy()
    return out[0][0].cpu().numpy(), out[1][0].cpu().numpy()


def hand_pose_from_window_keypoints(hand_model: HandModel, cameras: List[CameraModel], window_keypoints: np.ndarray,
                                    hand_idx: int, weights: Optional[np.ndarray] = None,
                                    init: Optional[SingleHandPose] = None, use_information: bool = False,
                                    refine_in_views: bool = False, loss="squared", loss_scale: float = 3.0,
                                    return_uncertainty: bool = False) -> tuple:
    """From 2-D detections to a pose: window_keypoints [n_cams,21,2] of one hand in the cameras -> (SingleHandPose, the
    triangulation's info [21,4]).  triangulate_landmarks first, then the pose fit of hand_pose_from_landmarks with each
    landmark weighted by (smallest finite sigma / its sigma)^2, in (0, 1]: a landmark the views pin down badly counts
    less; refused and degenerate landmarks count 0.  weights [n_cams,21], init and hand_confidence as for
    triangulate_landmarks / hand_pose_from_landmarks.  use_information=True: the triangulation hands its 3 x 3 information
    per landmark to the fit instead (hand.fit_landmarks_info) - triangulation with factor, the isotropic fit on the
    landmarks that carry information (from `init` when given), then the information fit started from it - so that depth,
    which a narrow baseline measures badly, is fixed by the hand's known size.  refine_in_views=True: the pose of either
    chain is then refined on ALL given detections by refine_hand_pose_in_views - the landmarks that one camera alone sees, which
    the triangulation refuses, included; the default leaves the chain's result as it is.  loss, loss_scale: the
    refinement's, as for refine_hand_pose_in_views; not read without it.  return_uncertainty=True: a third item, the
    hand.PoseUncertainty of the returned pose on ALL given detections under loss / loss_scale (hand_pose_uncertainty_in_views)."""
    pose, info = _chain_pose_from_window_keypoints(hand_model, cameras, window_keypoints, hand_idx, weights, init, use_information)
    if refine_in_views:
        pose = refine_hand_pose_in_views(hand_model, cameras, window_keypoints, hand_idx, pose, weights, loss=loss, loss_scale=loss_scale)[0]
    if return_uncertainty:
        return pose, info, hand_pose_uncertainty_in_views(hand_model, cameras, window_keypoints, hand_idx, pose, weights, loss, loss_scale)
    return pose, info


def hand_pose_uncertainty_in_views(hand_model: HandModel, cameras: List[CameraModel], window_keypoints: np.ndarray, hand_idx: int,
                                   pose: SingleHandPose, weights: Optional[np.ndarray] = None, loss="squared", loss_scale: float = 3.0,
                                   angle_sigma=None):
    """How well `pose` is known from the detections window_keypoints [n_cams,21,2] of one hand in the cameras: the
    hand.PoseUncertainty of hand.pose_uncertainty_views (numpy fields), one ut_pose_information_views launch.  weights [n_cams,21]
    are informations (1 / sigma^2 in px^-2 makes the result absolute; None = per px^2 of detection noise), loss / loss_scale those
    of the fit that produced the pose, angle_sigma [20] rad an optional prior on the joint angles.  Cameras as for
    triangulate_landmarks."""
    table, win, weights = _window_inputs("hand_pose_uncertainty_in_views", cameras, window_keypoints, weights, (len(cameras), 21, 2))
    unc = pose_uncertainty_views(
        hand_model, *_start_tensors(pose), torch.from_numpy(win), torch.arange(len(cameras), dtype=torch.int32), torch.from_numpy(table),
        weights=None if weights is None else torch.from_numpy(weights), angle_sigma=angle_sigma, loss=loss, loss_scale=loss_scale,
        mirror=_mirror_flag(hand_idx))
    return type(unc)(*(t.numpy() for t in unc))


def smooth_hand_poses_in_views(hand_model: HandModel, cameras: List[List[CameraModel]], window_keypoints: np.ndarray, hand_idx: int,
                               init: SingleHandPose, step_sigma, weights: Optional[np.ndarray] = None, loss="squared",
                               loss_scale: float = 3.0, frame_weight: Optional[np.ndarray] = None, centre=None):
    """One hand through T frames of detections, fitted frame by frame and then smoothed over the sequence: cameras[t] the cameras
    of frame t (the same number in every frame), window_keypoints [T,n_cams,21,2], weights [T,n_cams,21] informations (1 / sigma^2
    in px^-2 of each detection, 0 where the camera does not see the landmark; None = all 1, and then step_sigma is in units of the
    detection noise).  Frame t is fitted by refine_hand_pose_in_views from frame t - 1's fit (frame 0 from `init`), as
    hand_poses_from_keypoints warm-starts its frames; then ONE ut_pose_information_views launch at the T fits and ONE
    ut_smooth_pose_sequence launch (hand.smooth_poses: step_sigma [26] per frame step - hand.step_sigma_from_rates -, frame_weight
    [T], centre).  A frame whose fit is refused carries no information and is filled in from its neighbours.  Returns (the T
    smoothed SingleHandPoses with the fits' hand_confidence, info [T,4] and param_sigma [T,26] of hand.smooth_poses)."""
    win = np.ascontiguousarray(window_keypoints, np.float64)
    frames = len(cameras)
    if frames == 0 or win.ndim != 4 or win.shape[0] != frames:
        raise ValueError(f"window_keypoints must be [{frames},n_cams,21,2] for {frames} frames of cameras, got {win.shape}")
    n_cams = win.shape[1]
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float32)
    tables = [_window_inputs("smooth_hand_poses_in_views", cameras[t], win[t], None if weights is None else weights[t], (n_cams, 21, 2))[0]
              for t in range(frames)]
    ja, xf, fit_info = _track_one_sequence(hand_model, win, tables, hand_idx, init, None, weights, loss, loss_scale, RECOVER_RATIO)[:3]
    poses = [_pose_from_fit(ja[t], xf[t], fit_info[t]) for t in range(frames)]
    rows = torch.arange(frames * n_cams, dtype=torch.int32).reshape(frames, n_cams)
    mirror = _mirror_flag(hand_idx)
    unc = pose_uncertainty_views(hand_model, ja, xf, torch.from_numpy(win), rows, torch.from_numpy(np.concatenate(tables)),
                                 weights=None if weights is None else torch.from_numpy(weights), loss=loss, loss_scale=loss_scale,
                                 mirror=mirror.expand(frames))
    sja, sxf, info, sigma = smooth_poses(hand_model, ja, xf, unc, step_sigma, mirror=mirror, centre=centre, return_sigma=True,
                                         frame_weight=None if frame_weight is None else torch.from_numpy(np.ascontiguousarray(frame_weight, np.float32)))
    out = [SingleHandPose(joint_angles=sja[t].numpy(), wrist_xform=sxf[t].numpy(), hand_confidence=poses[t].hand_confidence) for t in range(frames)]
    return out, info.numpy(), sigma.numpy()


def refine_hand_pose_in_views(hand_model: HandModel, cameras: List[CameraModel], window_keypoints: np.ndarray, hand_idx: int,
                              init: SingleHandPose, weights: Optional[np.ndarray] = None, loss="squared", loss_scale: float = 3.0,
                              return_uncertainty: bool = False):
    """The pose that meets the detections themselves: window_keypoints [n_cams,21,2] of one hand in the cameras and a start
    `init` (the previous frame's pose, or hand_pose_from_window_keypoints') -> (SingleHandPose, info [4]: rms reprojection
    residual px, largest reprojection distance px, iterations, status bits FIT_*, residual [n_cams,21]: the reprojection
    distance of every used detection), one ut_fit_pose_views launch (hand.fit_landmarks_views, csrc/fit_views.hip).  weights
    [n_cams,21] >= 0, 0 where the camera does not see the landmark (the window there is not read); None = all 1.  One camera
    is enough: the hand's known size fixes its depth.  Cameras as for triangulate_landmarks.  loss "huber" / "geman_mcclure" with
    loss_scale px: the robust cost of hand.fit_landmarks_views, for detections some of which are grossly wrong (a fingertip on the
    wrong finger); a fourth item then, inlier [n_cams,21]: psi of every used detection at the returned pose, 1 an inlier, towards
    0 an outlier.  The default "squared" returns the three items it always did.  return_uncertainty=True: a last item more, the
    hand.PoseUncertainty of the returned pose under the same loss, weights and views (hand_pose_uncertainty_in_views)."""
    table, win, weights = _window_inputs("refine_hand_pose_in_views", cameras, window_keypoints, weights, (len(cameras), 21, 2))
    robust = _native.loss_code(loss) != _native.UT_LOSS_SQUARED
    ja, xf, fit_info, residual, *inlier = fit_landmarks_views(
        hand_model, torch.from_numpy(win), torch.arange(len(cameras), dtype=torch.int32), torch.from_numpy(table), _start_tensors(init),
        weights=None if weights is None else torch.from_numpy(weights), mirror=_mirror_flag(hand_idx),
        with_residual=True, loss=loss, loss_scale=loss_scale, return_inliers=robust)
    pose = _pose_from_fit(ja, xf, fit_info)
    out = (pose, fit_info.numpy(), residual.numpy()) + tuple(r.numpy() for r in inlier)
    if return_uncertainty:
        out += (hand_pose_uncertainty_in_views(hand_model, cameras, win, hand_idx, pose, weights, loss, loss_scale),)
    return out


def hand_pose_from_window_keypoints_cold(hand_model: HandModel, cameras: List[CameraModel], window_keypoints: np.ndarray,
                                         hand_idx: int, weights: Optional[np.ndarray] = None, loss="squared", loss_scale: float = 3.0):
    """From 2-D detections to a pose with no start at all, one camera being enough: window_keypoints [n_cams,21,2] of one hand in
    the cameras -> (SingleHandPose, info [4] of the chosen fit: rms reprojection residual px, largest reprojection distance px,
    iterations, status bits FIT_*, the chosen row of hand.start_pose_bank or -1).  hand.fit_landmarks_views_cold: the starts of
    csrc/start_views.hip, the fit in the views from each, the best kept.  weights, loss, loss_scale and cameras as for
    refine_hand_pose_in_views.  A hand seen from one side only can end in a mirror pose of nearly the same picture; the rms says so
    only when a second camera sees it."""
    table, win, weights = _window_inputs("hand_pose_from_window_keypoints_cold", cameras, window_keypoints, weights, (len(cameras), 21, 2))
    ja, xf, fit_info, index = fit_landmarks_views_cold(
        hand_model, torch.from_numpy(win), torch.arange(len(cameras), dtype=torch.int32), torch.from_numpy(table),
        weights=None if weights is None else torch.from_numpy(weights), mirror=_mirror_flag(hand_idx), loss=loss, loss_scale=loss_scale)
    return _pose_from_fit(ja, xf, fit_info), fit_info.numpy(), int(index)


def track_hand_poses_in_views(hand_model: HandModel, cameras: List[List[CameraModel]], window_keypoints: np.ndarray, hand_idx: int,
                              init: Optional[SingleHandPose] = None, recover_ratio: float = RECOVER_RATIO,
                              weights: Optional[np.ndarray] = None, loss="squared", loss_scale: float = 3.0):
    """One hand through T frames of detections with a way back after a loss: cameras[t] the cameras of frame t (the same number in
    every frame), window_keypoints [T,n_cams,21,2], weights [T,n_cams,21] or None.  The cold chain of
    hand_pose_from_window_keypoints_cold runs for all T frames as ONE batch (three launches).  Then, in ONE ut_track_pose_views launch
    (hand.track_landmarks_views), frame by frame the warm fit of refine_hand_pose_in_views from the previous frame's choice - frame
    0 from `init`, or the cold result when init is None.  A frame keeps its warm fit unless that is refused or its rms exceeds
    recover_ratio x the cold rms + RECOVER_FLOOR_PX: then the cold result is taken (if it is not refused itself), and the next frame
    starts from it.  recover_ratio must be finite and at least 1 (the C entry takes no infinity: a ratio such as 1e30 recovers on a
    refused fit alone).  Returns (the T SingleHandPoses, info [T,4] of the chosen fits, recovered [T] bool: the frames that took the
    cold result)."""
    win = np.ascontiguousarray(window_keypoints, np.float64)
    frames = len(cameras)
    if frames == 0 or win.ndim != 4 or win.shape[0] != frames:
        raise ValueError(f"window_keypoints must be [{frames},n_cams,21,2] for {frames} frames of cameras, got {win.shape}")
    if not 1.0 <= recover_ratio < float("inf"):
        raise ValueError(f"recover_ratio must be at least 1 and finite, got {recover_ratio}")
    n_cams = win.shape[1]
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float32)
    tables = [_window_inputs("track_hand_poses_in_views", cameras[t], win[t], None if weights is None else weights[t], (n_cams, 21, 2))[0]
              for t in range(frames)]
    rows = torch.arange(frames * n_cams, dtype=torch.int32).reshape(frames, n_cams)
    cja, cxf, cinfo, cindex = fit_landmarks_views_cold(
        hand_model, torch.from_numpy(win), rows, torch.from_numpy(np.concatenate(tables)),
        weights=None if weights is None else torch.from_numpy(weights), mirror=_mirror_flag(hand_idx).expand(frames), loss=loss,
        loss_scale=loss_scale)
    ja, xf, info, chosen = _track_one_sequence(hand_model, win, tables, hand_idx, init, (cja, cxf, cinfo, cindex), weights, loss, loss_scale,
                                               recover_ratio)
    return [_pose_from_fit(ja[t], xf[t], info[t]) for t in range(frames)], info.numpy(), (chosen == TRACK_COLD).numpy()


def _track_one_sequence(hand_model, win, tables, hand_idx, init, cold, weights, loss, loss_scale, recover_ratio):
    """hand.track_landmarks_views on one hand's T frames: win [T,n_cams,21,2], tables the T frames' camera tables, init a
    SingleHandPose or None, cold the four results of fit_landmarks_views_cold on the same rows or None."""
    frames, n_cams = win.shape[:2]
    rows = torch.arange(frames * n_cams, dtype=torch.int32).reshape(frames, n_cams)
    return track_landmarks_views(hand_model, torch.from_numpy(win), rows, torch.from_numpy(np.concatenate(tables)), _start_tensors(init), cold,
                                 weights=None if weights is None else torch.from_numpy(weights), mirror=_mirror_flag(hand_idx), loss=loss,
                                 loss_scale=loss_scale, recover_ratio=recover_ratio, recover_floor=RECOVER_FLOOR_PX)


def _chain_pose_from_window_keypoints(hand_model, cameras, window_keypoints, hand_idx, weights, init, use_information):
    """hand_pose_from_window_keypoints without the refinement in the views."""
    if use_information:
        pts, info, factor = triangulate_landmarks(cameras, window_keypoints, weights, with_information=True)
    else:
        pts, info = triangulate_landmarks(cameras, window_keypoints, weights)
    if pts.shape[0] != 21:
        raise ValueError(f"window_keypoints must be [{len(cameras)},21,2], got {np.shape(window_keypoints)}")
    if use_information:
        flip = _mirror_flag(hand_idx)
        target, used = torch.from_numpy(pts.astype(np.float32)), torch.from_numpy((factor != 0).any(-1).astype(np.float32))
        start = _start_tensors(init)
        if start is not None:
            start = fit_landmarks(hand_model, target, weights=used, init=start, mirror=flip)[:2]
        return _pose_from_fit(*fit_landmarks_info(hand_model, target, torch.from_numpy(factor), init=start, mirror=flip)), info
    sigma = info[:, 1].astype(np.float64)
    ok = np.isfinite(sigma) & (sigma > 0)
    lw = np.zeros(21, np.float32)
    if ok.any():
        lw[ok] = (sigma[ok].min() / sigma[ok]) ** 2
    return _pose_from_fit(*fit_landmarks(hand_model, torch.from_numpy(pts.astype(np.float32)), weights=torch.from_numpy(lw),
                                         init=_start_tensors(init), mirror=_mirror_flag(hand_idx))), info


def calibrate_hand_model_from_keypoints(hand_model: HandModel, keypoints: np.ndarray, valid: np.ndarray,
                                        n_calibration_samples: int = 0) -> Tuple[HandModel, float, np.ndarray]:
    """A model scaled to the person whose 3-D keypoints these are: the keypoint twin of the reference's calibration pass
    (run_eval_unknown_skeleton.py:55-76, which averages the network's predicted scales and applies scaled_hand_model).
    keypoints [n_hands, n_frames, 21, 3] (mm, world; hand 1 is the right hand) and valid [n_hands, n_frames] in the layout
    of the eval result files; hand_model e.g. the generic one.  Every valid hand-frame is fitted with a free scale, both
    hands pool into one scale (hand.calibrate_scale) - samples in the reference's order, frame by frame and hand by hand,
    only the first n_calibration_samples valid ones when that is not 0.  Invalid hand-frames get weight 0: the fit refuses
    them and the pool leaves them out.  Returns (scaled_hand_model(hand_model, scale), scale, stats [4]: scale, sigma,
    scatter, poses used - see hand.ScaleCalibration).  ValueError when no pose is usable."""
    keypoints, valid = np.asarray(keypoints), np.asarray(valid, bool)
    n_hands, n_frames = valid.shape
    if keypoints.shape != (n_hands, n_frames, 21, 3):
        raise ValueError(f"keypoints must be [{n_hands},{n_frames},21,3], got {keypoints.shape}")
    use = valid.T.reshape(-1).copy()                                        # frame major, like the reference's sample list
    if n_calibration_samples:
        use &= np.cumsum(use) <= n_calibration_samples
    kp = np.where(use[:, None, None], keypoints.transpose(1, 0, 2, 3).reshape(-1, 21, 3), 0).astype(np.float32)
    w = np.repeat(use[:, None], 21, 1).astype(np.float32)
    mirror = np.tile((np.arange(n_hands) == RIGHT_HAND_INDEX).astype(np.int64), n_frames)
    cal = calibrate_scale(hand_model, torch.from_numpy(kp), torch.from_numpy(w), torch.from_numpy(mirror), refit=False)
    return cal.hand_model, float(cal.scale), cal.stats.numpy()


def calibrate_hand_model_from_window_keypoints(hand_model: HandModel, cameras: List[CameraModel], window_keypoints: np.ndarray,
                                               hand_idx: int, weights: Optional[np.ndarray] = None, refine_in_views: bool = False,
                                               loss="squared", loss_scale: float = 3.0) -> ScaleCalibration:
    """From 2-D detections to a calibrated model: window_keypoints [n_frames, n_cams, 21, 2] of one hand in the cameras,
    weights [n_frames, n_cams, 21] as for triangulate_landmarks -> hand.ScaleCalibration (its hand_model is the calibrated
    model, its poses are refitted at the calibrated scale).  One ut_triangulate_points launch for all frames, each
    landmark weighted as in hand_pose_from_window_keypoints - (the frame's smallest finite sigma / its sigma)^2 -, then
    hand.calibrate_scale over the frames.  refine_in_views=True: that chain's free pass - its poses and per-pose scales - is
    the start of hand.calibrate_scale_in_views on ALL given detections (free pass in the views -> pool -> fixed pass in the
    views), which roughly halves the scale's error on the same detections and keeps the frames the 3-D chain cannot use; sigma
    and scatter of the result are then per px.  loss, loss_scale: the passes' in the views, as for refine_hand_pose_in_views; not
    read without refine_in_views.  The cameras must see the hand from two places: one camera cannot see its size."""
    table, win, weights = _window_inputs("calibrate_hand_model_from_window_keypoints", cameras, window_keypoints, weights,
                                         ("n_frames", len(cameras), 21, 2))
    dev = fk_device()
    n = win.shape[0]
    rows = torch.arange(len(cameras), dtype=torch.int32, device=dev)[None].expand(n, -1).contiguous()
    pts, info, _ = _native.triangulate_points(torch.from_numpy(win).to(dev), rows, torch.from_numpy(table).to(dev),
                                              weights=None if weights is None else torch.from_numpy(weights).to(dev))
    sigma = info[..., 1].double()
    ok = torch.isfinite(sigma) & (sigma > 0)
    best = torch.where(ok, sigma, torch.full_like(sigma, float("inf"))).amin(1, keepdim=True)
    lw = torch.where(ok, (best / torch.where(ok, sigma, torch.ones_like(sigma))) ** 2, torch.zeros_like(sigma)).float()
    mirror = torch.full((n,), 1 if hand_idx == RIGHT_HAND_INDEX else 0, dtype=torch.int64, device=dev)
    if refine_in_views:
        start = calibrate_scale(hand_model, pts.float(), lw, mirror, refit=False)
        cal = calibrate_scale_in_views(hand_model, torch.from_numpy(win).to(dev), rows, torch.from_numpy(table).to(dev),
                                       (start.joint_angles, start.wrist_transforms), start.pose_scale,
                                       weights=None if weights is None else torch.from_numpy(weights).to(dev), mirror=mirror,
                                       loss=loss, loss_scale=loss_scale)
    else:
        cal = calibrate_scale(hand_model, pts.float(), lw, mirror)
    return ScaleCalibration(*(t.cpu() if isinstance(t, torch.Tensor) else t for t in cal))


def _visible_counts(cameras: List[CameraModel], landmarks_world: np.ndarray) -> List[int]:
    counts = []
    for cam in cameras:
        eye = cam.world_to_eye(landmarks_world)
        win = cam.eye_to_window(eye)
        inside = ((win[..., 0] >= 0) & (win[..., 0] <= cam.width - 1) & (win[..., 1] >= 0)
                  & (win[..., 1] <= cam.height - 1) & (eye[..., 2] > 0))
        counts.append(int(inside.sum()))
    return counts


def _rank_by_visibility(counts: List[int], min_required_vis_landmarks: int) -> List[int]:
    """The cameras that see enough landmarks, most first; equal counts keep index order (perspective_crop.py:78-86)."""
    keep = [i for i, n in enumerate(counts) if n >= min_required_vis_landmarks]
    keep.sort(reverse=True, key=lambda i: counts[i])
    return keep


def rank_hand_visibility_in_cameras(cameras, hand_model, hand_pose, hand_idx, min_required_vis_landmarks) -> List[int]:
    counts = _visible_counts(cameras, landmarks_from_hand_pose(hand_model, hand_pose, hand_idx))
    return _rank_by_visibility(counts, min_required_vis_landmarks)


def _pose_stack_landmarks(hand_model: HandModel, poses: List[np.ndarray], wrist_xform: np.ndarray, hand_idx: int
                          ) -> np.ndarray:
    """FK of several joint-angle vectors under one wrist transform in ONE kernel launch: [len(poses),21,3]."""
    ja = np.stack([np.asarray(p, np.float32) for p in poses])
    xf = np.broadcast_to(_left_handed(wrist_xform, hand_idx).astype(np.float32), (len(poses), 4, 4))
    # an unbatched model is shared by all poses of the launch (ut_fk n_models == 1)
    return skin_landmarks_np(hand_model, ja, np.ascontiguousarray(xf))


def _get_crop_points_from_hand_pose(hand_model, gt_hand_pose, hand_idx, num_crop_points) -> np.ndarray:
    assert num_crop_points in [21, 42, 63]
    poses = [gt_hand_pose.joint_angles]
    if num_crop_points > 21:
        poses.append(neutral_joint_angles(hand_model).numpy())
    if num_crop_points > 42:
        poses.append(np.zeros(NUM_JOINTS_PER_HAND, dtype=np.float32))
    return _pose_stack_landmarks(hand_model, poses, gt_hand_pose.wrist_xform, hand_idx).reshape(-1, 3)


def gen_crop_cameras_from_pose(cameras, camera_angles, hand_model, hand_pose, hand_idx, num_crop_points,
                               new_image_size, max_view_num: Optional[int] = None, sort_camera_index: bool = False,
                               focal_multiplier: float = 0.95, mirror_right_hand: bool = True,
                               min_required_vis_landmarks: int = 19) -> Dict[int, PinholePlaneCameraModel]:
    """Pick the best views of one hand and aim a 96x96 pinhole crop camera at it from each
    (lib/tracker/perspective_crop.py:136-180).  The first 21 crop points are the landmarks of the pose
    itself, so the visibility ranking re-uses them instead of running FK again."""
    crop_points = _get_crop_points_from_hand_pose(hand_model, hand_pose, hand_idx, num_crop_points)
    order = _rank_by_visibility(_visible_counts(cameras, crop_points[:21]), min_required_vis_landmarks)
    if sort_camera_index:
        order = sorted(order)
    out: Dict[int, PinholePlaneCameraModel] = {}
    for ci in order:
        out[ci] = geometry.gen_crop_parameters_from_points(
            cameras[ci], crop_points, new_image_size, mirror_img_x=(mirror_right_hand and hand_idx == 1),
            camera_angle=camera_angles[ci], focal_multiplier=focal_multiplier)
        if len(out) == max_view_num:
            break
    return out


def crop_camera_from_window_points(camera: CameraModel, window_hand_pose: np.ndarray, hand_idx: int, input_size,
                                   hand_ratio_in_crop: float) -> PinholePlaneCameraModel:
    """One (hand, camera) of HandTracker.gen_crop_cameras_from_stereo_camera_with_window_hand_pose
    (lib/tracker/tracker.py:128-176): unproject the 21 window keypoints through the camera's own window_to_eye (for
    Fisheye62 the radial-only five-step fixed point, lib/common/camera.py:146-181), aim a crop camera at their
    bounding-box centre (camera angle 0, x-mirrored for hand 1) and fit its focal length to them.  Raises
    ValueError("Unable to create crop camera", ...) where the reference does (lib/common/crop.py:25-26)."""
    world_to_eye = np.linalg.inv(camera.camera_to_world_xf)
    world = camera.eye_to_world(camera.window_to_eye(np.asarray(window_hand_pose)[:, :2]))
    center = (world.min(axis=0) + world.max(axis=0)) / 2
    new_world_to_eye = geometry.make_look_at_matrix(world_to_eye, center, 0)
    if hand_idx == 1:
        mirrorx = np.eye(4, dtype=np.float32)
        mirrorx[0, 0] = -1
        new_world_to_eye = mirrorx @ new_world_to_eye
    fx_fy, cx_cy = geometry.gen_intrinsics_from_bounding_pts(geometry.transform3(new_world_to_eye, world),
                                                             input_size[0], input_size[1])
    return PinholePlaneCameraModel(width=input_size[0], height=input_size[1], f=hand_ratio_in_crop * fx_fy, c=cx_cy,
                                   distort_coeffs=[], camera_to_world_xf=np.linalg.inv(new_world_to_eye))


def gen_crop_cameras_from_window_points(camera_left: CameraModel, camera_right: CameraModel,
                                        window_hand_pose_left: Dict[int, np.ndarray],
                                        window_hand_pose_right: Dict[int, np.ndarray], input_size,
                                        hand_ratio_in_crop: float) -> Dict[int, Dict[int, PinholePlaneCameraModel]]:
    """Host path of gen_crop_cameras_from_stereo_camera_with_window_hand_pose (lib/tracker/tracker.py:111-219), any
    camera model: the left dict's hands in insertion order with view key 0, then the right dict's views as key 1 (a
    hand seen only on the right is appended)."""
    out: Dict[int, Dict[int, PinholePlaneCameraModel]] = {}
    for view, camera, hands in ((0, camera_left, window_hand_pose_left), (1, camera_right, window_hand_pose_right)):
        for hand_idx, pose in hands.items():
            cam = crop_camera_from_window_points(camera, pose, hand_idx, input_size, hand_ratio_in_crop)
            out.setdefault(hand_idx, {})[view] = cam
    return out


def _crop_camera_from_row(row: np.ndarray, k: np.ndarray, ext: np.ndarray, size: int) -> PinholePlaneCameraModel:
    """A crop camera as a crop-camera kernel returned it (crop_params row, K, world->eye in metres)."""
    t = np.eye(4)
    t[:3, :3] = row[4:13].reshape(3, 3)
    t[:3, 3] = row[13:16]
    cam = PinholePlaneCameraModel(width=size, height=size, f=(row[0], row[1]), c=(row[2], row[3]), distort_coeffs=[],
                                  camera_to_world_xf=t)
    # what _make_inputs needs of this camera, as the kernel computed it (row, K, world->eye in metres)
    cam._ut_net = (row, k, ext)
    return cam


# What both crop-camera kernels return per candidate, under the keys of their `out=` dict: (key, dtype, shape).
_CROP_OUT_FIELDS = (("crop_params", np.float64, (MAX_VIEW_NUM, 24)), ("intrinsics", np.float32, (MAX_VIEW_NUM, 9)),
                    ("extrinsics", np.float32, (MAX_VIEW_NUM, 16)), ("cam_index", np.int32, (MAX_VIEW_NUM,)),
                    ("n_views", np.int32, ()), ("status", np.int32, ()))


def _crop_out_stage_fields(*extra):
    """_Stage output fields of NUM_HANDS candidates: _CROP_OUT_FIELDS (and `extra`, same form), one row per candidate."""
    return [(key, dtype, (NUM_HANDS,) + shape) for key, dtype, shape in _CROP_OUT_FIELDS + extra]


def _crop_out_dict(stage: "_Stage", n: int) -> Dict[str, torch.Tensor]:
    """The `out=` dict of a crop-camera launch of n candidates: the first n rows of every staged output field."""
    return {key: t[:n] for key, t in stage.t_out.items()}


def _crop_cameras_from_rows(o: Dict[str, np.ndarray], i: int, size: int) -> Dict[int, PinholePlaneCameraModel]:
    """{source camera: crop camera} of candidate i from the read-back rows `o` (keys of _CROP_OUT_FIELDS), slot order."""
    return {int(o["cam_index"][i, k]): _crop_camera_from_row(o["crop_params"][i, k].copy(), o["intrinsics"][i, k].copy(),
                                                             o["extrinsics"][i, k].copy(), size)
            for k in range(int(o["n_views"][i]))}


# ----------------------------------------------------------------------------- tracker.py
@dataclass
class ViewData:
    image: np.ndarray
    camera: CameraModel
    camera_angle: float


@dataclass
class InputFrame:
    views: List[ViewData]


@dataclass
class HandTrackerOpts:
    num_crop_points: int = 63
    enable_memory: bool = True
    use_stored_pose_for_crop: bool = True
    hand_ratio_in_crop: float = 0.8
    min_required_vis_landmarks: int = 19


def network_camera_inputs(crop_camera: PinholePlaneCameraModel) -> Tuple[np.ndarray, np.ndarray]:
    """K [3,3] and world->eye extrinsics with the translation in metres (lib/tracker/tracker.py:333-337)."""
    ext = np.linalg.inv(crop_camera.camera_to_world_xf)
    ext[:3, 3] *= MM_TO_M
    return crop_camera.uv_to_window_matrix(), ext


def _net_inputs(crop_camera: PinholePlaneCameraModel):
    """(packed crop row f64[24], K, world->eye in metres) of a crop camera: as ut_gen_crop_cameras computed them when the
    camera came from the batched generator and still holds those parameters, else from the host formulas."""
    net = getattr(crop_camera, "_ut_net", None)
    if net is not None:
        row, t = net[0], crop_camera.camera_to_world_xf
        if (row[0], row[1], row[2], row[3]) == (crop_camera.f[0], crop_camera.f[1], crop_camera.c[0], crop_camera.c[1]) \
                and np.array_equal(row[4:13].reshape(3, 3), t[:3, :3]) and np.array_equal(row[13:16], t[:3, 3]):
            return net
    k, ext = network_camera_inputs(crop_camera)
    return geometry.pack_camera_model(crop_camera), k, ext


# ----------------------------------------------------------------------------- per-frame staging
_TORCH_DTYPE = {np.dtype(k): v for k, v in ((np.uint8, torch.uint8), (np.int32, torch.int32), (np.int64, torch.int64),
                                            (np.float32, torch.float32), (np.float64, torch.float64))}


def _stage_layout(fields):
    """({name: (byte offset, dtype, shape)}, total bytes) of `fields` = [(name, dtype, shape)] laid out in order, every
    field starting on a 16-byte boundary."""
    layout, off = {}, 0
    for name, dtype, shape in fields:
        layout[name] = (off, dtype, shape)
        off += (int(np.prod(shape)) * np.dtype(dtype).itemsize + 15) // 16 * 16
    return layout, off


def _stage_views(buf, layout):
    """{name: typed view of the field's bytes} over a flat uint8 buffer, a numpy array or a tensor."""
    views = {}
    for name, (off, dtype, shape) in layout.items():
        raw = buf[off: off + int(np.prod(shape)) * np.dtype(dtype).itemsize]
        views[name] = raw.view(dtype if isinstance(buf, np.ndarray) else _TORCH_DTYPE[np.dtype(dtype)]).reshape(shape)
    return views


_MAX_CAMS = 8       # source cameras the gen_crop_cameras staging holds


def _crop_stage_fields():
    """(inputs, outputs) of gen_crop_cameras' staging."""
    return ([("cam", np.float64, (_MAX_CAMS, 32)), ("angles", np.float64, (_MAX_CAMS,)), ("ja", np.float32, (NUM_HANDS, 22)),
             ("xf", np.float32, (NUM_HANDS, 16)), ("frame", np.int32, (NUM_HANDS,)), ("hand", np.int64, (NUM_HANDS,))],
            _crop_out_stage_fields(("landmarks", np.float32, (21, 3))))


def _window_stage_fields():
    """(inputs, outputs) of the window-keypoint crop cameras' staging."""
    return ([("cam", np.float64, (2, 32)), ("kp", np.float64, (NUM_HANDS, MAX_VIEW_NUM, 21, 2)),
             ("src_row", np.int32, (NUM_HANDS, MAX_VIEW_NUM)), ("hand", np.int64, (NUM_HANDS,))], _crop_out_stage_fields())


def _frame_stage_fields(hgt: int, wid: int):
    """(inputs, outputs) of track_frame's staging for source images of hgt x wid; the images come last, so that an
    upload can stop after the ones in use."""
    nc, ns = NUM_HANDS * MAX_VIEW_NUM, NUM_HANDS
    return ([("cam", np.float64, (4, 32)), ("crop", np.float64, (nc, 24)), ("src_index", np.int32, (nc,)),
             ("k", np.float32, (nc, 3, 3)), ("ext", np.float32, (nc, 4, 4)), ("range", np.int64, (ns, 2)),
             ("mem", np.int64, (ns,)), ("hand", np.int64, (ns,)), ("use", np.uint8, (ns,)),
             ("skel", np.float32, (1, 2, 22, 3)), ("img", np.uint8, (4, hgt, wid))],
            [("pose", np.float32, (ns, 60)), ("kp", np.float32, (ns, 21, 3)), ("status", np.int32, (2,))])


class _Stage:
    """One pinned host buffer + its device mirror with a fixed layout: everything a call needs goes up in ONE
    host->device copy and everything it returns comes back in ONE device->host copy (the per-frame API otherwise
    spends its time in dozens of tiny transfers, each a stream synchronisation)."""

    def __init__(self, dev: torch.device, fields_in, fields_out):
        self.dev = dev
        self.in_off, self.in_bytes = _stage_layout(fields_in)
        self.out_off, self.out_bytes = _stage_layout(fields_out)
        self.h_in = torch.empty(self.in_bytes, dtype=torch.uint8).pin_memory()
        self.d_in = torch.empty(self.in_bytes, dtype=torch.uint8, device=dev)
        self.h_out = torch.empty(self.out_bytes, dtype=torch.uint8).pin_memory()
        self.d_out = torch.empty(self.out_bytes, dtype=torch.uint8, device=dev)
        self.np_in, self.t_in = _stage_views(self.h_in.numpy(), self.in_off), _stage_views(self.d_in, self.in_off)
        self.np_out, self.t_out = _stage_views(self.h_out.numpy(), self.out_off), _stage_views(self.d_out, self.out_off)

    def upload(self, n_bytes: Optional[int] = None):
        n = self.in_bytes if n_bytes is None else n_bytes
        self.d_in[:n].copy_(self.h_in[:n], non_blocking=True)

    def download(self):
        self.h_out.copy_(self.d_out, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()


class _LandmarkMemo:
    """(Process-wide, not thread-safe - like the reference, which runs one tracker per process.)
    landmarks_from_hand_pose is a pure function of (hand model, pose, hand index); gen_crop_cameras and track_frame
    already run that FK on the GPU for the poses the eval scripts ask about next (run_eval_known_skeleton.py:84-89), so
    they leave the results here.  An entry is used only when the pose arrays are bit-identical and the model tensors are
    the same objects at the same in-place version."""

    def __init__(self, cap: int = 16):
        self.cap = cap
        self.items = []       # (model tensors, hand_idx, joint_angles f32[22], wrist f32[4,4], landmarks [21,3])

    def put(self, hand_model, hand_idx, ja, xf, kp):
        self.items.insert(0, (tuple((t, t._version) for t in (getattr(hand_model, f) for f in _MEMO_FIELDS)), int(hand_idx),
                              np.array(ja, np.float32), np.array(xf, np.float32), np.array(kp, np.float32)))
        del self.items[self.cap:]

    def get(self, hand_model, hand_idx, ja, xf):
        ja32, xf32 = np.asarray(ja, np.float32), np.asarray(xf, np.float32)
        if ja32.shape != (NUM_JOINTS_PER_HAND,) or xf32.shape != (4, 4):
            return None
        for model, h, j, x, kp in self.items:
            if h == int(hand_idx) and np.array_equal(j, ja32) and np.array_equal(x, xf32) and \
                    all(a is b and v == b._version for (a, v), b in zip(model, (getattr(hand_model, f) for f in _MEMO_FIELDS))):
                return kp.copy()
        return None


_MEMO_FIELDS = ("joint_rotation_axes", "joint_rest_positions", "landmark_rest_positions", "landmark_rest_bone_weights",
                "landmark_rest_bone_indices")
_landmark_memo = _LandmarkMemo()


class HandTracker:
    def __init__(self, model, opts: HandTrackerOpts) -> None:
        self._device: str = "cuda" if torch.cuda.device_count() else "cpu"
        logger.info(f"Using device: {self._device}")
        self._model = model
        self._model.to(self._device)
        self._input_size = np.array(self._model.getInputImageSizes())
        self._num_crop_points = opts.num_crop_points
        self._enable_memory = opts.enable_memory
        self._hand_ratio_in_crop: float = opts.hand_ratio_in_crop
        self._min_required_vis_landmarks: int = opts.min_required_vis_landmarks
        self._valid_tracking_history = np.zeros(2, dtype=bool)
        self._remap_mode = _native.UT_REMAP_CV2_FIXED
        self._crop_stage: Optional[_Stage] = None       # staging of gen_crop_cameras (one upload, one read-back)
        self._window_stage: Optional[_Stage] = None     # staging of gen_crop_cameras_from_stereo_camera_with_window_hand_pose
        self._frame_stage: Optional[_Stage] = None      # staging of track_frame
        self._frame_stage_key = None
        self._limits_dev = None                         # (joint_limits tensor identity, device copy)

    def reset_history(self) -> None:
        self._valid_tracking_history[:] = False

    def _engine(self):
        """The model's native engine.  The tracker feeds it one frame (<= 4 crops) at a time and switches it to latency
        mode for the duration of each of its own calls (`eng.modes(...)`), so a batched user of the same handle keeps
        the default dispatch."""
        return self._model.engine

    def gen_crop_cameras(self, cameras: List[CameraModel], camera_angles: List[float], hand_model: HandModel,
                         gt_tracking: Dict[int, SingleHandPose], min_num_crops: int
                         ) -> Dict[int, Dict[int, PinholePlaneCameraModel]]:
        crop_cameras: Dict[int, Dict[int, PinholePlaneCameraModel]] = {}
        hands = [(h, p) for h, p in (gt_tracking or {}).items() if p.hand_confidence >= CONFIDENCE_THRESHOLD]
        if hands and self._device == "cuda" and self._batched_cropgen_ok(cameras, hand_model):
            out = self._gen_crop_cameras_batched(cameras, camera_angles, hand_model, hands, min_num_crops)
            if out is not None:
                return out
        for hand_idx, pose in (gt_tracking or {}).items():
            if pose.hand_confidence < CONFIDENCE_THRESHOLD:
                continue
            per_hand = gen_crop_cameras_from_pose(
                cameras, camera_angles, hand_model, pose, hand_idx, self._num_crop_points, self._input_size,
                max_view_num=MAX_VIEW_NUM, sort_camera_index=True, focal_multiplier=self._hand_ratio_in_crop,
                mirror_right_hand=True, min_required_vis_landmarks=self._min_required_vis_landmarks)
            if per_hand and len(per_hand) >= min_num_crops:
                crop_cameras[hand_idx] = per_hand
        return crop_cameras

    def _batched_cropgen_ok(self, cameras, hand_model) -> bool:
        """ut_gen_crop_cameras covers the configuration the eval scripts use: 63 crop points, square crops, Fisheye62
        source cameras of one size, an unbatched hand model with joint limits."""
        return (self._num_crop_points == 63 and self._input_size[0] == self._input_size[1] and len(cameras) > 0
                and all(isinstance(c, geometry.Fisheye62CameraModel) for c in cameras)
                and len({(c.width, c.height) for c in cameras}) == 1
                and hand_model.joint_limits is not None and hand_model.joint_rest_positions.dim() == 2)

    def _gen_crop_cameras_batched(self, cameras, camera_angles, hand_model, hands, min_num_crops):
        """All hands of the frame through one ut_gen_crop_cameras launch (lib/tracker/tracker.py:222-260): one
        staged upload (camera rows + poses), one launch, one read-back.  The launch also returns the landmarks of
        every pose; they are remembered for landmarks_from_hand_pose (the eval scripts ask for them next)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        n, nc, v = len(hands), len(cameras), MAX_VIEW_NUM
        if n > NUM_HANDS or nc > _MAX_CAMS:
            return None
        st = self._crop_stage
        if st is None or st.dev != dev:
            st = self._crop_stage = _Stage(dev, *_crop_stage_fields())
            st.np_in["frame"][:] = 0
        a = st.np_in
        for ci, cam in enumerate(cameras):
            a["cam"][ci] = geometry.pack_camera_model(cam)
        a["angles"][:nc] = np.asarray(camera_angles, np.float64)
        for i, (h, pose) in enumerate(hands):
            a["ja"][i] = np.asarray(pose.joint_angles, np.float32)
            a["xf"][i] = np.asarray(pose.wrist_xform, np.float32).reshape(16)
            a["hand"][i] = h
        st.upload()
        lim = hand_model.joint_limits
        if self._limits_dev is None or self._limits_dev[0] is not lim:
            self._limits_dev = (lim, lim.float().contiguous().to(dev))
        blob = device_blob(hand_model, dev)
        ti = st.t_in
        # (the staged frame index is always 0 and the hands come from the caller's dict: no index read-back)
        _native.gen_crop_cameras(
            ti["cam"][:nc], ti["angles"][:nc], blob, self._limits_dev[1], ti["ja"][:n], ti["xf"][:n], ti["frame"][:n],
            ti["hand"][:n], nc, (cameras[0].width, cameras[0].height), max_views=v,
            min_vis=self._min_required_vis_landmarks, crop_size=int(self._input_size[0]),
            focal_multiplier=self._hand_ratio_in_crop, check_indices=False, want_landmarks=True,
            out=_crop_out_dict(st, n))
        st.download()                                                         # one read-back
        o = st.np_out
        crop_cameras: Dict[int, Dict[int, PinholePlaneCameraModel]] = {}
        size = int(self._input_size[0])
        for i, (hand_idx, pose) in enumerate(hands):
            if int(o["status"][i]) != 0:
                raise ValueError("Unable to create crop camera")
            _landmark_memo.put(hand_model, hand_idx, pose.joint_angles, pose.wrist_xform, o["landmarks"][i])
            per_hand = _crop_cameras_from_rows(o, i, size)
            if per_hand and len(per_hand) >= min_num_crops:
                crop_cameras[hand_idx] = per_hand
        return crop_cameras

    def gen_crop_cameras_from_stereo_camera_with_window_hand_pose(
            self, camera_left: CameraModel, camera_right: CameraModel, window_hand_pose_left: Dict[int, np.ndarray],
            window_hand_pose_right: Dict[int, np.ndarray]) -> Dict[int, Dict[int, PinholePlaneCameraModel]]:
        """Crop cameras from 2-D hand keypoints of a stereo pair (lib/tracker/tracker.py:111-219, the live demo's
        path): window_hand_pose_* map a hand index to its 21 window keypoints [21, >=2] (only [:, :2] is read).
        Returns {hand: {0: left crop camera, 1: right crop camera}} in the reference's key order.  Fisheye62 cameras
        on a HIP device: every hand of both cameras in one ut_gen_crop_cameras_from_window_points launch (one staged
        upload, one read-back); anything else runs the host path.  Raises ValueError("Unable to create crop
        camera") where the reference raises."""
        left, right = window_hand_pose_left or {}, window_hand_pose_right or {}
        hands = list(left) + [h for h in right if h not in left]
        if hands and self._device == "cuda" and self._window_cropgen_ok(camera_left, camera_right, left, right, hands):
            return self._gen_crop_cameras_from_window_batched(camera_left, camera_right, left, right, hands)
        return gen_crop_cameras_from_window_points(camera_left, camera_right, left, right, self._input_size,
                                                   self._hand_ratio_in_crop)

    def _window_cropgen_ok(self, camera_left, camera_right, left, right, hands) -> bool:
        """The kernel's configuration: Fisheye62 cameras, square crops, hands 0 / 1, 21 keypoints per hand."""
        return (self._input_size[0] == self._input_size[1] and len(hands) <= NUM_HANDS
                and all(isinstance(c, geometry.Fisheye62CameraModel) for c in (camera_left, camera_right))
                and all(h in (0, 1) for h in hands)
                and all(np.ndim(p) == 2 and np.shape(p)[0] == 21 and np.shape(p)[1] >= 2
                        for d in (left, right) for p in d.values()))

    def _gen_crop_cameras_from_window_batched(self, camera_left, camera_right, left, right, hands):
        dev = torch.device("cuda", torch.cuda.current_device())
        st = self._window_stage
        if st is None or st.dev != dev:
            st = self._window_stage = _Stage(dev, *_window_stage_fields())
        a = st.np_in
        a["cam"][0] = geometry.pack_camera_model(camera_left)
        a["cam"][1] = geometry.pack_camera_model(camera_right)
        for i, h in enumerate(hands):
            a["hand"][i] = h
            for view, d in enumerate((left, right)):
                if h in d:
                    a["kp"][i, view] = np.asarray(d[h])[:, :2]
                    a["src_row"][i, view] = view
                else:
                    a["src_row"][i, view] = -1
        st.upload()
        ti, n = st.t_in, len(hands)
        # (_window_cropgen_ok vetted the hands and the rows are 0 / 1 / -1; the C entry checks the indices again itself)
        _native.gen_crop_cameras_from_window_points(
            ti["cam"], ti["kp"][:n], ti["src_row"][:n], ti["hand"][:n], crop_size=int(self._input_size[0]),
            focal_multiplier=self._hand_ratio_in_crop, check_indices=False, out=_crop_out_dict(st, n))
        st.download()                                                         # one read-back
        o = st.np_out
        if (o["status"][:n] != 0).any():
            raise ValueError("Unable to create crop camera")
        size = int(self._input_size[0])
        return {h: _crop_cameras_from_rows(o, i, size) for i, h in enumerate(hands)}

    # ------------------------------------------------------------------ network inputs
    def _make_inputs(self, sample: InputFrame, hand_model_mm: Optional[HandModel], crop_cameras):
        """Resample every (hand, view) crop on the GPU and assemble the network inputs
        (lib/tracker/tracker.py:315-368).  Dict order defines the sample order."""
        dev = torch.device(self._device)
        if dev.type != "cuda":
            raise _native.NativeLibraryError("HandTracker needs a HIP device: the crop resampler and the network "
                                             "have no CPU fallback")
        used_cams = sorted({ci for per_hand in crop_cameras.values() for ci in per_hand})
        slot_of = {ci: i for i, ci in enumerate(used_cams)}
        src = torch.from_numpy(np.stack([np.ascontiguousarray(sample.views[ci].image) for ci in used_cams])).to(dev)
        cam_rows = np.stack([geometry.pack_camera_model(sample.views[ci].camera) for ci in used_cams])
        crop_rows, src_index, intrinsics, extrinsics, sample_range, hand_indices = [], [], [], [], [], []
        for hand_idx, per_hand in crop_cameras.items():
            start = len(crop_rows)
            for cam_idx, crop_camera in per_hand.items():
                row, k, ext = _net_inputs(crop_camera)
                crop_rows.append(row)
                src_index.append(slot_of[cam_idx])
                intrinsics.append(np.asarray(k, np.float64).reshape(3, 3))
                extrinsics.append(np.asarray(ext, np.float64).reshape(4, 4))
            if len(crop_rows) > start:
                hand_indices.append(hand_idx)
                sample_range.append((start, len(crop_rows)))
        hand_indices = np.array(hand_indices)
        crops = self._engine().warp_crops(
            src, torch.from_numpy(cam_rows).to(dev), torch.from_numpy(np.stack(crop_rows)).to(dev),
            torch.tensor(src_index, dtype=torch.int32, device=dev), self._remap_mode)
        frame_data = InputFrameData(
            left_images=crops,
            intrinsics=torch.from_numpy(np.stack(intrinsics)).float().to(dev),
            extrinsics_xf=torch.from_numpy(np.stack(extrinsics)).float().to(dev))
        frame_desc = InputFrameDesc(
            sample_range=torch.tensor(sample_range, dtype=torch.long, device=dev),
            memory_idx=torch.from_numpy(hand_indices).long().to(dev),
            use_memory=torch.from_numpy(self._valid_tracking_history[hand_indices]).bool().to(dev),
            hand_idx=torch.from_numpy(hand_indices).long().to(dev))
        skeleton_data = None
        if hand_model_mm is not None:
            hand_model_m = scaled_hand_model(hand_model_mm, MM_TO_M)
            skeleton_data = InputSkeletonData(
                joint_rotation_axes=hand_model_m.joint_rotation_axes.float().to(dev),
                joint_rest_positions=hand_model_m.joint_rest_positions.float().to(dev))
        return frame_data, frame_desc, skeleton_data

    def _run_staged(self, sample, hand_model, crop_cameras, calibrate: bool) -> Optional[TrackingResult]:
        """track_frame with ONE upload (images + every parameter row), the launches (resample + backbone, head, FK of
        the regressed poses) and ONE read-back.  Returns None when the frame does not fit the staging layout (more than
        two hands / four crops, images that are not contiguous u8 of one size): the general path then runs."""
        dev = torch.device("cuda", torch.cuda.current_device())
        n_crops = sum(len(v) for v in crop_cameras.values())
        if len(crop_cameras) > NUM_HANDS or n_crops > NUM_HANDS * MAX_VIEW_NUM or any(len(v) == 0 for v in crop_cameras.values()):
            return None
        used = sorted({ci for per_hand in crop_cameras.values() for ci in per_hand})
        imgs = [sample.views[ci].image for ci in used]
        hgt, wid = imgs[0].shape[:2]
        if len(used) > 4 or any(im.dtype != np.uint8 or im.shape != (hgt, wid) for im in imgs):
            return None
        key = (str(dev), hgt, wid)
        st = self._frame_stage
        if st is None or self._frame_stage_key != key:
            nc = NUM_HANDS * MAX_VIEW_NUM
            st = self._frame_stage = _Stage(dev, *_frame_stage_fields(hgt, wid))
            self._frame_stage_key = key
            self._feat = torch.empty(nc, 72, 6, 6, device=dev)
            self._engine().reserve(nc, NUM_HANDS, NUM_HANDS)
        a = st.np_in
        slot_of = {ci: i for i, ci in enumerate(used)}
        for i, ci in enumerate(used):
            a["cam"][i] = geometry.pack_camera_model(sample.views[ci].camera)
            a["img"][i] = imgs[i]
        n = s = 0
        hands = []
        for hand_idx, per_hand in crop_cameras.items():
            start = n
            for cam_idx, crop_camera in per_hand.items():
                net = _net_inputs(crop_camera)
                a["crop"][n] = net[0]
                a["k"][n] = np.asarray(net[1], np.float32).reshape(3, 3)
                a["ext"][n] = np.asarray(net[2], np.float32).reshape(4, 4)
                a["src_index"][n] = slot_of[cam_idx]
                n += 1
            a["range"][s] = (start, n)
            a["mem"][s] = a["hand"][s] = hand_idx
            a["use"][s] = self._valid_tracking_history[hand_idx]
            hands.append(hand_idx)
            s += 1
        if hand_model is not None:     # mm -> m (lib/tracker/tracker.py:361-367)
            a["skel"][0, 0] = hand_model.joint_rotation_axes.numpy()
            a["skel"][0, 1] = hand_model.joint_rest_positions.numpy() * np.float32(MM_TO_M)
        st.upload(st.in_off["img"][0] + len(used) * hgt * wid)
        eng, ti, to = self._engine(), st.t_in, st.t_out
        mode = _native.UT_MODE_UNKNOWN if calibrate else _native.UT_MODE_KNOWN
        all_multiview = all(len(v) == MAX_VIEW_NUM for v in crop_cameras.values())
        if calibrate and not all_multiview:
            raise AssertionError("Unsupported: found single-view samples when calibration scale")
        blob = None if hand_model is None else device_blob(hand_model, dev)
        n_used, n_slots = len(used), max(hands) + 1

        # (Replaying the sequence as a captured hipGraph was measured in round 2: no gain - the loop is bound by the ~0.9 ms of
        # GPU time, not by the ~65 launches; the launches stay eager.  The whole-path replay hang of that experiment was the
        # library's hipMemsetAsync nodes: see csrc/ut_kernels.h::launch_zero_words.)
        # deferred checks: every index tensor above was built here, nothing to wait for in mid-sequence; the verdict
        # rides in the one read-back below (a set bit means the device skipped the head: the poses would be stale)
        with eng.modes(deferred_checks=True, latency=True):
            feat = eng.warp_backbone(ti["img"][:n_used], ti["cam"][:n_used], ti["crop"][:n], ti["src_index"][:n],
                                     self._remap_mode, out=self._feat[:n])
            pose, _ = eng.fuse_temporal_regress(feat, ti["k"][:n], ti["ext"][:n], ti["range"][:s], ti["mem"][:s],
                                                ti["use"][:s], ti["hand"][:s], n_slots, all_multiview,
                                                None if calibrate else ti["skel"], mode, out=to["pose"][:s])
            if blob is not None:
                eng.fk(blob, pose, pose[:, 22:], mirror=ti["hand"][:s], t_scale=M_TO_MM, ja_stride=60, xf_stride=60,
                       n=s, out=to["kp"][:s])
            eng.status_snapshot(to["status"])
        st.download()                                                         # one read-back
        o = st.np_out
        if o["status"][0] != 0:
            eng.poll_status()                                                 # raises for the failed check, clears it
        rec = o["pose"][:s]
        res = self._tracking_result(hands, rec[:, :22].copy(), rec[:, 22:38].reshape(s, 4, 4).copy(),
                                    rec[:, 38].copy() if calibrate else None, crop_cameras)
        if not calibrate and hand_model is not None:
            for i, hand_idx in enumerate(hands):
                pose_i = res.hand_poses[hand_idx]
                _landmark_memo.put(hand_model, hand_idx, pose_i.joint_angles, pose_i.wrist_xform, o["kp"][i])
        return res

    def _run(self, sample, hand_model, crop_cameras, calibrate: bool) -> TrackingResult:
        if not crop_cameras:
            self.reset_history()       # frame without hands
            return TrackingResult()
        if self._device == "cuda" and (calibrate or (hand_model is not None and hand_model.joint_rest_positions.dim() == 2
                                                     and hand_model.joint_rest_positions.device.type == "cpu"
                                                     and hand_model.joint_rotation_axes.device.type == "cpu")):
            res = self._run_staged(sample, hand_model, crop_cameras, calibrate)
            if res is not None:
                return res
        frame_data, frame_desc, skeleton_data = self._make_inputs(sample, hand_model, crop_cameras)
        scope = self._engine().modes(latency=True) if self._device == "cuda" else contextlib.nullcontext()
        with scope:        # a frame's few crops: latency dispatch for this call only
            if calibrate:
                out = self._model.regress_pose_pred_skel_scale(frame_data, frame_desc)
            else:
                out = self._model.regress_pose_use_skeleton(frame_data, frame_desc, skeleton_data)
        return self._gen_tracking_result(out, frame_desc.hand_idx.cpu().numpy(), crop_cameras)

    def track_frame(self, sample: InputFrame, hand_model: HandModel, crop_cameras) -> TrackingResult:
        return self._run(sample, hand_model, crop_cameras, calibrate=False)

    def track_frame_analysis(self, sample: InputFrame, hand_model: HandModel, crop_cameras,
                             gt_tracking: Optional[Dict[int, SingleHandPose]]) -> TrackingResult:
        """lib/tracker/tracker.py:416-604, the live demo's call: the body is track_frame's (the same warp with the
        depth check, the same TrackingResult, the same validity-history update), so is this one.  gt_tracking is
        accepted and ignored, as in the reference.  The reference also shows every crop with cv2.imshow /
        cv2.waitKey(1); that GUI side effect is not reproduced (OpenCV's GUI is not a dependency here)."""
        return self.track_frame(sample, hand_model, crop_cameras)

    def track_frame_and_calibrate_scale(self, sample: InputFrame, crop_cameras) -> TrackingResult:
        return self._run(sample, None, crop_cameras, calibrate=True)

    def _gen_tracking_result(self, regressor_output: RegressorOutput, hand_indices: np.ndarray, crop_cameras
                             ) -> TrackingResult:
        scales = None if regressor_output.skel_scales is None else regressor_output.skel_scales.to("cpu").numpy()
        return self._tracking_result(hand_indices, regressor_output.joint_angles.to("cpu").numpy(),
                                     regressor_output.wrist_xfs.to("cpu").numpy(), scales, crop_cameras)

    def _tracking_result(self, hands, ja: np.ndarray, xf: np.ndarray, scales: Optional[np.ndarray], crop_cameras
                         ) -> TrackingResult:
        """m -> mm, per-hand dicts, validity history (lib/tracker/tracker.py:370-412).  Row i of ja [S,22], xf [S,4,4]
        (metres; scaled in place, the caller hands over arrays of its own) and scales [S] (or None) belongs to hands[i]."""
        xf[..., :3, 3] *= M_TO_MM
        hand_poses, num_views, predicted_scales = {}, {}, {}
        for i, hand_idx in enumerate(hands):
            hand_poses[hand_idx] = SingleHandPose(joint_angles=ja[i], wrist_xform=xf[i], hand_confidence=1.0)
            num_views[hand_idx] = len(crop_cameras[hand_idx])
            if scales is not None:
                predicted_scales[hand_idx] = scales[i]
        for hand_idx in range(NUM_HANDS):
            self._valid_tracking_history[hand_idx] = hand_idx in hand_poses
        return TrackingResult(hand_poses=hand_poses, num_views=num_views, predicted_scales=predicted_scales)
