"""Hand model container and forward kinematics entry points with the reference's names
(lib/common/hand.py:11-147, lib/common/hand_skinning.py:189-209).

`skin_landmarks` is part of the hot path: it always runs the HIP
kernel csrc/fk.hip through the C ABI - inputs on the CPU are moved to the GPU and the result is
returned on the input's device.  There is no CPU implementation in the product.
"""
from enum import Enum
from typing import Any, Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _native

NUM_HANDS = 2
NUM_LANDMARKS_PER_HAND = 21
NUM_FINGERTIPS_PER_HAND = 5
NUM_JOINTS_PER_HAND = 22
LEFT_HAND_INDEX = 0
RIGHT_HAND_INDEX = 1
NUM_DIGITS = 5
NUM_JOINT_FRAMES = 1 + 1 + 3 * 5
DOF_PER_FINGER = 4


class LANDMARK(Enum):
    THUMB_FINGERTIP = "Thumb fingertip"
    INDEX_FINGER_FINGERTIP = "Index finger fingertip"
    MIDDLE_FINGER_FINGERTIP = "Middle finger fingertip"
    RING_FINGER_FINGERTIP = "Ring finger fingertip"
    PINKY_FINGER_FINGERTIP = "Pinky finger fingertip"
    WRIST_JOINT = "Wrist joint"
    THUMB_INTERMEDIATE_FRAME = "Thumb intermediate frame"
    THUMB_DISTAL_FRAME = "Thumb distal frame"
    INDEX_PROXIMAL_FRAME = "Index proximal frame"
    INDEX_INTERMEDIATE_FRAME = "Index intermediate frame"
    INDEX_DISTAL_FRAME = "Index distal frame"
    MIDDLE_PROXIMAL_FRAME = "Middle proximal frame"
    MIDDLE_INTERMEDIATE_FRAME = "Middle intermediate frame"
    MIDDLE_DISTAL_FRAME = "Middle distal frame"
    RING_PROXIMAL_FRAME = "Ring proximal frame"
    RING_INTERMEDIATE_FRAME = "Ring intermediate frame"
    RING_DISTAL_FRAME = "Ring distal frame"
    PINKY_PROXIMAL_FRAME = "Pinky proximal frame"
    PINKY_INTERMEDIATE_FRAME = "Pinky intermediate frame"
    PINKY_DISTAL_FRAME = "Pinky distal frame"
    PALM_CENTER = "Palm center"


class HandModel(NamedTuple):
    joint_rotation_axes: torch.Tensor
    joint_rest_positions: torch.Tensor
    joint_frame_index: torch.Tensor
    joint_parent: torch.Tensor
    joint_first_child: torch.Tensor
    joint_next_sibling: torch.Tensor
    landmark_rest_positions: torch.Tensor
    landmark_rest_bone_weights: torch.Tensor
    landmark_rest_bone_indices: torch.Tensor
    hand_scale: Optional[torch.Tensor]
    mesh_vertices: Optional[torch.Tensor] = None
    mesh_triangles: Optional[torch.Tensor] = None
    dense_bone_weights: Optional[torch.Tensor] = None
    joint_limits: Optional[torch.Tensor] = None

    @classmethod
    def from_json(cls, json_data: Dict[str, Any]) -> "HandModel":
        return cls(**{k: (torch.tensor(v) if v is not None else None) for k, v in json_data.items()})

    def to_json(self) -> Dict[str, Any]:
        return {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in self._asdict().items()}


def _lead_factor(hand: HandModel, multiplier) -> torch.Tensor:
    lead = hand.joint_rest_positions.shape[:-2]
    ones = torch.ones(lead, dtype=hand.joint_rest_positions.dtype, device=hand.joint_rest_positions.device)
    return (ones * multiplier)[..., None, None]


def scaled_hand_model(hand: HandModel, multiplier) -> HandModel:
    """Scale every length of the model (lib/common/hand.py:78-111)."""
    m = _lead_factor(hand, multiplier)
    return hand._replace(
        joint_rest_positions=hand.joint_rest_positions * m,
        landmark_rest_positions=hand.landmark_rest_positions * m,
        mesh_vertices=None if hand.mesh_vertices is None else hand.mesh_vertices * m,
    )


def mirrored_hand_model(hand: HandModel, to_mirror: torch.Tensor) -> HandModel:
    """Left<->right mirror of the selected models: x of positions and y,z of rotation axes change sign
    (lib/common/hand.py:114-147; mesh vertices are left untouched there too)."""
    sel = to_mirror.reshape(-1).to(torch.bool)
    lead = to_mirror.shape

    def flip(t: torch.Tensor, cols: slice) -> torch.Tensor:
        out = t.clone()
        flat = out.reshape((-1,) + t.shape[len(lead):])
        sub = flat[sel]
        sub[..., cols] = -sub[..., cols]
        flat[sel] = sub
        return flat.reshape(t.shape)

    return hand._replace(
        joint_rotation_axes=flip(hand.joint_rotation_axes, slice(1, None)),
        joint_rest_positions=flip(hand.joint_rest_positions, slice(0, 1)),
        landmark_rest_positions=flip(hand.landmark_rest_positions, slice(0, 1)),
        mesh_vertices=None if hand.mesh_vertices is None else hand.mesh_vertices.clone(),
    )


_fk_engine_handles: Dict[int, "_native.HipEngine"] = {}


def fk_device() -> torch.device:
    if not torch.cuda.is_available():
        raise _native.NativeLibraryError(
            "skin_landmarks runs on the HIP kernel csrc/fk.hip and no HIP device is visible "
            "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


_BLOB_FIELDS = ("joint_rotation_axes", "joint_rest_positions", "landmark_rest_positions", "landmark_rest_bone_weights",
                "landmark_rest_bone_indices")
_blob_cache: list = []      # [(key, tensors kept alive, device blob)], most recent first


def device_blob(hand_model: HandModel, dev: torch.device) -> torch.Tensor:
    """The packed [n_models, 321] fp32 model the FK / crop-camera kernels read, cached on the device: the per-frame
    API skins the same HandModel several times per frame.  Keyed on tensor identity + in-place version counters."""
    tensors = tuple(getattr(hand_model, f) for f in _BLOB_FIELDS)
    key = (str(dev),) + tuple((id(t), t._version) for t in tensors)
    for i, (k, _keep, blob) in enumerate(_blob_cache):
        if k == key:
            if i:
                _blob_cache.insert(0, _blob_cache.pop(i))
            return blob
    blob = torch.from_numpy(_native.hand_model_blob(*tensors).reshape(-1, 321)).to(dev)
    _blob_cache.insert(0, (key, tensors, blob))
    del _blob_cache[8:]
    return blob


def skin_landmarks(hand_model: HandModel, joint_angles: torch.Tensor, wrist_transforms: torch.Tensor) -> torch.Tensor:
    """[...,22] joint angles + [...,4,4] wrist transforms -> [...,21,3] landmarks, any leading dims; the
    model's tensors are either unbatched or carry the same leading dims (lib/common/hand_skinning.py:189-209)."""
    lead = tuple(joint_angles.shape[:-1])
    n = int(np.prod(lead)) if lead else 1
    model_lead = tuple(hand_model.joint_rest_positions.shape[:-2])
    if model_lead not in ((), lead):
        raise AssertionError(f"Leading dimensions do not match, got {lead} and {model_lead}")
    src_device = joint_angles.device
    dev = src_device if src_device.type == "cuda" else fk_device()
    out = _native.fk_stateless(device_blob(hand_model, dev),
                               joint_angles.reshape(n, 22).to(dev, torch.float32),
                               wrist_transforms.reshape(n, 4, 4).to(dev, torch.float32))
    return out.reshape(lead + (21, 3)).to(src_device)


FIT_CONVERGED, FIT_AT_MAX_ITERS, FIT_REFUSED = _native.UT_FIT_CONVERGED, _native.UT_FIT_AT_MAX_ITERS, _native.UT_FIT_REFUSED


class _FitStaging:
    """How the fit_landmarks* wrappers stage a call: the model checked against the leading dims `lead` of the landmarks (or
    windows), `limits` against the model (`limits_word`: how the wrapper's message names the argument), the device the kernel
    runs on, the model blob and the box there; f32 / flags flatten an argument to n poses on that device, back gives a result
    its leading dims again on the source device.  broadcast: arguments are first expanded to the leading dims, so a number or
    one row stands for all poses - fit_landmarks_scale and calibrate_scale alone."""

    def __init__(self, hand_model: HandModel, lead, src_device, limits, limits_word="limits=True", broadcast=False):
        self.lead, self.n, self.src_device, self.broadcast = lead, int(np.prod(lead)) if lead else 1, src_device, broadcast
        model_lead = tuple(hand_model.joint_rest_positions.shape[:-2])
        if model_lead not in ((), lead):
            raise AssertionError(f"Leading dimensions do not match, got {lead} and {model_lead}")
        if limits and hand_model.joint_limits is None:
            raise ValueError(f"{limits_word} needs hand_model.joint_limits")
        self.dev = src_device if src_device.type == "cuda" else fk_device()
        self.box = hand_model.joint_limits[..., :20, :].reshape(-1, 20, 2).to(self.dev, torch.float32) if limits else None
        self.blob = device_blob(hand_model, self.dev)

    def f32(self, t, tail, dtype=torch.float32):
        if t is None:
            return None
        if self.broadcast:
            t = torch.as_tensor(t).expand(self.lead + tail)
        return t.reshape((self.n,) + tail).to(self.dev, dtype)

    def flags(self, mirror):
        return self.f32(mirror, (), torch.int64)

    def init(self, init):
        return (None, None) if init is None else (self.f32(init[0], (22,)), self.f32(init[1], (4, 4)))

    def back(self, t, tail):
        return t.reshape(self.lead + tail).to(self.src_device)


def _views_staging(hand_model: HandModel, window, cam_rows, table, weights, limits):
    """How the wrappers on detections in V views stage a call: window [...,V,21,2] checked -> (the _FitStaging on its leading
    dims, V, (window f64 [n,V,21,2], cam_rows i32 [n,V], table f64) on the device, weights [n,V,21] there or None)."""
    if window.dim() < 3 or tuple(window.shape[-2:]) != (21, 2):
        raise ValueError(f"window must be [...,V,21,2], got {tuple(window.shape)}")
    v = window.shape[-3]
    s = _FitStaging(hand_model, tuple(window.shape[:-3]), window.device, limits, "limits")
    views = (s.f32(window, (v, 21, 2), torch.float64), s.f32(cam_rows, (v,), torch.int32), table.to(s.dev, torch.float64))
    return s, v, views, s.f32(weights, (v, 21))


def fit_landmarks(hand_model: HandModel, landmarks: torch.Tensor, weights: Optional[torch.Tensor] = None, init=None,
                  limits: bool = False, mirror: Optional[torch.Tensor] = None, max_iters: int = 32):
    """The inverse of skin_landmarks: [...,21,3] landmarks -> (joint_angles [...,22], wrist_transforms [...,4,4], info
    [...,4]) with skin_landmarks(hand_model, joint_angles, wrist_transforms) ~ landmarks, on the HIP kernel csrc/fit.hip (no
    CPU implementation; the reference has no such function).  Leading dims and devices as for skin_landmarks: the skeleton
    fields are unbatched or carry the landmarks' leading dims, inputs on the CPU are moved to the GPU and the results come
    back on the landmarks' device.  weights [...,21] >= 0: how much each landmark counts; the landmarks of weight 0 are
    not read (they may be NaN).  init = (joint_angles [...,22], wrist_transforms [...,4,4]) warm-starts the fit, None
    starts from the rest pose aligned to the landmarks.  limits=True keeps the angles inside hand_model.joint_limits
    (fewer than half of the recorded label poses lie inside them, so this is off by default); otherwise angles come back
    in (-pi, pi].  mirror [...] of 0 / 1 as for skin_mesh: where 1, the landmarks are those of a right hand and the
    returned transform is the proper one a pose holds (column 0 is negated by the consumer).  info: weighted rms residual,
    worst residual, iterations, status - FIT_CONVERGED | FIT_AT_MAX_ITERS | FIT_REFUSED (fewer than 3 weighted landmarks,
    a bad weight or a non-finite weighted landmark: the pose is the init, or the rest pose)."""
    s = _FitStaging(hand_model, tuple(landmarks.shape[:-2]), landmarks.device, limits)
    ja, xf, info = _native.fit_pose(s.blob, s.f32(landmarks, (21, 3)), s.f32(weights, (21,)), s.box, *s.init(init), s.flags(mirror),
                                    max_iters=max_iters)
    return s.back(ja, (22,)), s.back(xf, (4, 4)), s.back(info, (4,))


def fit_landmarks_info(hand_model: HandModel, landmarks: torch.Tensor, sqrt_info: torch.Tensor, init=None, limits: bool = False,
                       mirror: Optional[torch.Tensor] = None, max_iters: int = 32):
    """fit_landmarks for landmarks that come with their information, on the HIP kernel csrc/fit_info.hip (no CPU
    implementation): sqrt_info [...,21,6] holds (l00, l10, l11, l20, l21, l22) of the lower Cholesky factor L of each
    landmark's 3 x 3 information matrix - what tracker.triangulate_landmarks(..., with_information=True) returns, or
    chol(covariance^-1) of a depth sensor's or a motion capture system's landmarks - and the fit minimises sum_l |L_l^T
    (landmark_l - target_l)|^2 instead of treating a landmark's error as isotropic.  A landmark whose factor is all 0 is not used
    and may be NaN.  init = (joint_angles, wrist_transforms) warm-starts the fit; without one, fit_landmarks runs first on
    the used landmarks (weight 1, the others 0) and its result is the start - two launches, no host work between them: the
    anisotropic cost is flat along the viewing rays and a cold start on it can end in a local minimum.  Returns (joint_angles
    [...,22], wrist_transforms [...,4,4], info [...,4]: whitened rms residual - px for triangulated landmarks -, largest
    Euclidean residual, iterations, status as for fit_landmarks).  Everything else as for fit_landmarks."""
    lead = tuple(landmarks.shape[:-2])
    if tuple(sqrt_info.shape) != lead + (21, 6):
        raise ValueError(f"sqrt_info must be {lead + (21, 6)}, got {tuple(sqrt_info.shape)}")
    s = _FitStaging(hand_model, lead, landmarks.device, limits)
    targets, factor, flip = s.f32(landmarks, (21, 3)), s.f32(sqrt_info, (21, 6)), s.flags(mirror)
    if init is None:
        used = (factor != 0).any(-1).to(torch.float32)
        start = _native.fit_pose(s.blob, targets, used, s.box, mirror=flip, max_iters=max_iters)[:2]
    else:
        start = s.init(init)
    ja, xf, info = _native.fit_pose_info(s.blob, targets, factor, s.box, start[0], start[1], flip, max_iters=max_iters)
    return s.back(ja, (22,)), s.back(xf, (4, 4)), s.back(info, (4,))


def fit_landmarks_views(hand_model: HandModel, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor, init,
                        weights: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, limits=None,
                        max_iters: int = 32, with_residual: bool = False, loss="squared", loss_scale: float = 3.0,
                        return_inliers: bool = False):
    """fit_landmarks on 2-D keypoints in camera views instead of 3-D landmarks, on the HIP kernel csrc/fit_views.hip (no CPU
    implementation): the pose that minimises sum_v sum_l w_vl |project_v(landmark_l) - window_vl|^2 through the exact camera
    model.  window f64 [...,V,21,2] px; cam_rows i32 [...,V] rows of `table`, -1 = unused view; table f64 [R,32] Fisheye62
    source cameras or [R,24] pinhole crop cameras; weights [...,V,21] >= 0 or None = all 1 - a detection of weight 0 is not
    read and may be NaN.  Every detection counts, also of a landmark that one camera alone sees, and one view is enough.
    init = (joint_angles [...,22], wrist_transforms [...,4,4]) is required - the previous frame's pose, or fit_landmarks on
    the triangulated landmarks: without 3-D targets there is nothing to align a cold start to.  limits: true keeps the
    angles inside hand_model.joint_limits.  Returns (joint_angles [...,22], wrist_transforms [...,4,4], info [...,4]: rms
    reprojection residual px, largest reprojection distance px, iterations, status as for fit_landmarks) and, with
    with_residual=True, the reprojection distance [...,V,21] of every used detection - zero an outlier's weight and call
    again.  loss = "huber" or "geman_mcclure" fits the robust cost sum w c^2 rho(d^2 / c^2) with c = loss_scale px instead
    (_native.fit_pose_views_robust, csrc/fit_views_robust.hip): a few grossly wrong detections then cost one launch; info[0] is
    the robust cost's rms, the distances stay raw.  return_inliers=True appends psi [...,V,21] of every used detection at the
    returned pose - 1 an inlier, towards 0 an outlier; with the default "squared", which is the plain fit bit for bit, 1 at every
    used detection.  Leading dims, devices and mirror as for fit_landmarks."""
    if init is None:
        raise ValueError("init = (joint_angles, wrist_transforms) is required: fit_landmarks_views has no cold start")
    s, v, views, weights = _views_staging(hand_model, window, cam_rows, table, weights, limits)
    res = _native.fit_pose_views_any_loss(s.blob, *views, *s.init(init), weights, s.box, s.flags(mirror), max_iters=max_iters, loss=loss,
                                          loss_scale=loss_scale, residual=with_residual, inlier=return_inliers)
    out = (s.back(res[0], (22,)), s.back(res[1], (4, 4)), s.back(res[2], (4,)))
    return out + tuple(s.back(r, (v, 21)) for r in res[3:])


START_ITERS = 30      # rounds of the orthogonal iteration in cold_start_views


def start_pose_bank(hand_model: HandModel, fractions=(0.25, 0.5, 0.75)) -> torch.Tensor:
    """The finger poses cold_start_views tries, f32 [K,20]: the zero pose, then lo + f (hi - lo) of hand_model.joint_limits for
    every f in `fractions` (without joint_limits: the zero pose alone).  An unbatched skeleton, or the first of a batch."""
    bank = [torch.zeros(20, dtype=torch.float32)]
    if hand_model.joint_limits is not None and len(fractions):
        box = hand_model.joint_limits.reshape(-1, hand_model.joint_limits.shape[-2], 2)[0, :20].to("cpu", torch.float32)
        bank += [box[:, 0] + float(f) * (box[:, 1] - box[:, 0]) for f in fractions]
    return torch.stack(bank)


def start_rotation_seeds() -> torch.Tensor:
    """The 24 proper signed permutation matrices, f64 [24,3,3]: the rotations of the cube, in the order of the permutations
    (0,1,2), (0,2,1), ... and, within one, of the signs (+,+), (+,-), (-,+), (-,-) of the first two rows - the third follows
    from det = +1.  The identity is seed 0."""
    seeds = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        parity = 1.0 if perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1.0
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                q = np.zeros((3, 3))
                q[0, perm[0]], q[1, perm[1]], q[2, perm[2]] = s0, s1, parity * s0 * s1
                seeds.append(q)
    return torch.from_numpy(np.stack(seeds))


def cold_start_views(hand_model: HandModel, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                     weights: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, limits=None, bank=None,
                     seeds=None, iters: int = START_ITERS):
    """Starts for fit_landmarks_views from the detections alone, one launch of csrc/start_views.hip (no CPU implementation):
    per hand one start from each of the K finger poses of `bank` (default start_pose_bank(hand_model)), the hand moved rigidly
    onto the detections' rays from each of `seeds` (default start_rotation_seeds()) and the best seed kept by its reprojection
    cost.  window, cam_rows, table, weights, mirror, limits as for fit_landmarks_views.  Returns (joint_angles [...,K,22],
    wrist_transforms [...,K,4,4], info [...,K,4]: rms px, largest reprojection distance px, winning seed, status 0 or
    FIT_REFUSED)."""
    s, _v, views, weights = _views_staging(hand_model, window, cam_rows, table, weights, limits)
    bank = (start_pose_bank(hand_model) if bank is None else bank).to(s.dev, torch.float32)
    seeds = (start_rotation_seeds() if seeds is None else seeds).to(s.dev, torch.float64)
    k = bank.shape[0]
    ja, xf, info = _native.start_pose_views(s.blob, *views, bank, seeds, weights, s.box, s.flags(mirror), iters=iters)
    return s.back(ja, (k, 22)), s.back(xf, (k, 4, 4)), s.back(info, (k, 4))


def fit_landmarks_views_cold(hand_model: HandModel, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                             weights: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, limits=None,
                             max_iters: int = 32, loss="squared", loss_scale: float = 3.0, bank=None, seeds=None,
                             iters: int = START_ITERS):
    """fit_landmarks_views without an init: cold_start_views, then the fit from each of its K starts per hand (any `loss`), then
    the candidate with the lowest info[...,0] among those not refused (_native.select_pose) - three launches.  Returns
    (joint_angles [...,22], wrist_transforms [...,4,4], info [...,4]) as fit_landmarks_views does, plus the chosen candidate's
    index [...] (i32; -1 where every candidate was refused: the pose is then the first candidate's)."""
    s, _v, views, weights = _views_staging(hand_model, window, cam_rows, table, weights, limits)
    bank = (start_pose_bank(hand_model) if bank is None else bank).to(s.dev, torch.float32)
    seeds = (start_rotation_seeds() if seeds is None else seeds).to(s.dev, torch.float64)
    res = _cold_chain(s.blob, views, weights, s.box, s.flags(mirror), bank, seeds, iters, max_iters, loss, loss_scale)
    return s.back(res[0], (22,)), s.back(res[1], (4, 4)), s.back(res[2], (4,)), s.back(res[3], ())


TRACK_WARM, TRACK_COLD, TRACK_NONE = _native.UT_TRACK_WARM, _native.UT_TRACK_COLD, _native.UT_TRACK_NONE
RECOVER_RATIO = 1.5       # DESIGN.md, "Start of a pose fit in the views": warm rms / cold rms is 1.00 on the hand, 2.7 (median) once lost
RECOVER_FLOOR_PX = 0.01


def track_landmarks_views(hand_model: HandModel, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor, init=None, cold=None,
                          weights: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, limits=None,
                          lengths: Optional[torch.Tensor] = None, max_iters: int = 32, loss="squared", loss_scale: float = 3.0,
                          recover_ratio: float = RECOVER_RATIO, recover_floor: float = RECOVER_FLOOR_PX):
    """fit_landmarks_views through sequences of detections, on the HIP kernel csrc/track_views.hip (no CPU implementation): window
    f64 [...,T,V,21,2] holds T consecutive frames per sequence, cam_rows i32 [...,T,V], weights [...,T,V,21]; table, limits, loss and
    loss_scale as for fit_landmarks_views.  ONE launch follows every sequence through its frames: frame t is fitted from frame t - 1's
    result (frame 0 from init = (joint_angles [...,22], wrist_transforms [...,4,4]), one start per sequence) and keeps that warm fit
    unless it is refused or its rms exceeds recover_ratio x the cold rms + recover_floor px - then the cold result of the frame is
    taken, if it is not refused itself, and the next frame starts from it.  cold = (joint_angles [...,T,22], wrist_transforms
    [...,T,4,4], info [...,T,4], index [...,T]): what fit_landmarks_views_cold returns on the same window, or None: no recovery.
    init None: a sequence starts at its first usable cold result.  One of init and cold is needed.  mirror [...] or [...,T] of 0 /
    1; lengths i32 [...]: frames at or past a sequence's length are not fitted.  Returns (joint_angles [...,T,22], wrist_transforms
    [...,T,4,4], info [...,T,4] of the chosen fits, chosen i32 [...,T]: TRACK_WARM, TRACK_COLD - a recovery, or the first cold
    result of a sequence without an init -, TRACK_NONE - no start yet and a refused cold result, which the row then holds - and -1
    at or past the length).  The result is the per-frame chain of fit_landmarks_views bit for bit (include/umetrack_hip_track.h)."""
    if window.dim() < 4:
        raise ValueError(f"window must be [...,T,V,21,2], got {tuple(window.shape)}")
    s, _v, views, weights = _views_staging(hand_model, window, cam_rows, table, weights, limits)
    frames, seq_lead = s.lead[-1], s.lead[:-1]
    if frames < 1:
        raise ValueError("a sequence needs at least one frame")
    n_seq = s.n // frames
    if init is None and cold is None:
        raise ValueError("init or cold is needed: there is nothing to start from")
    if mirror is not None:
        mirror = torch.as_tensor(mirror)
        if tuple(mirror.shape) == seq_lead:
            mirror = mirror[..., None].expand(s.lead)
    start = (None, None) if init is None else (init[0].reshape(n_seq, 22).to(s.dev, torch.float32), init[1].reshape(n_seq, 4, 4).to(s.dev, torch.float32))
    if cold is not None:
        cold = (s.f32(cold[0], (22,)), s.f32(cold[1], (4, 4)), s.f32(cold[2], (4,)), s.f32(cold[3], (), torch.int32))
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(n_seq).to(s.dev, torch.int32)
    ja, xf, info, chosen = _native.track_pose_views(s.blob, *views, frames, start[0], start[1], cold, weights, s.box, s.flags(mirror), lengths,
                                                    max_iters=max_iters, loss=loss, loss_scale=loss_scale, recover_ratio=recover_ratio,
                                                    recover_floor=recover_floor)
    return s.back(ja, (22,)), s.back(xf, (4, 4)), s.back(info, (4,)), s.back(chosen, ())


def _cold_chain(blob, views, weights, box, mirror, bank, seeds, iters, max_iters, loss, loss_scale, t_scale: float = 1.0, engine=None):
    """start_pose_views -> fit_pose_views[_robust] on the n K starts -> select_pose, everything on the device: (joint_angles [n,22],
    wrist_xf [n,4,4], info [n,4], index i32 [n])."""
    k = bank.shape[0]
    window, cam_rows, table = views
    ja0, xf0, _ = _native.start_pose_views(blob, window, cam_rows, table, bank, seeds, weights, box, mirror, t_scale, iters, engine=engine)
    rep = (lambda t: t) if k == 1 else (lambda t: None if t is None else t.repeat_interleave(k, 0))
    many = (lambda t: t if t is None or t.shape[0] == 1 else rep(t))      # one model row stands for every pose
    ja, xf, info = _native.fit_pose_views_any_loss(many(blob), rep(window), rep(cam_rows), table, ja0, xf0, rep(weights), many(box),
                                                   rep(mirror), t_scale, max_iters, loss, loss_scale, engine=engine)[:3]
    return _native.select_pose(ja, xf, info, k)


COV_OK, COV_SINGULAR, COV_REFUSED = _native.UT_COV_OK, _native.UT_COV_SINGULAR, _native.UT_COV_REFUSED


class PoseUncertainty(NamedTuple):
    """How well a pose is known (pose_uncertainty_views).  The 26 parameters are the solver's: 20 joint angle increments (rad),
    a rotation increment about `pivot` in world axes (rad), a translation in the landmarks' units."""
    pose_info: torch.Tensor        # [...,26,26] H = sum w psi J^T J (+ the prior): the information matrix of the pose
    pivot: torch.Tensor            # [...,3] the point the rotation increment turns about
    param_sigma: torch.Tensor      # [...,26] sqrt(diag H^-1); +inf when singular
    landmark_cov: torch.Tensor     # [...,21,3,3] covariance of every landmark in the world; +inf on the diagonal when singular
    landmark_sigma: torch.Tensor   # [...,21] sqrt(trace landmark_cov)
    status: torch.Tensor           # [...] i64: COV_OK, COV_SINGULAR or COV_REFUSED (everything 0)


_TRIL = np.tril_indices(26)
_COV6 = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))


def unpack_uncertainty(pose_info, pivot, param_sigma, landmark_cov, info, lead=None, device=None) -> PoseUncertainty:
    """The five packed outputs of _native.pose_information_views ([n,351], [n,3], [n,26], [n,21,6], [n,4]) as a PoseUncertainty
    with leading dims `lead` (default (n,)) on `device` (default: where they are)."""
    n = pose_info.shape[0]
    lead = (n,) if lead is None else tuple(lead)
    h = pose_info.new_zeros(n, 26, 26)
    h[:, _TRIL[0], _TRIL[1]] = pose_info
    h[:, _TRIL[1], _TRIL[0]] = pose_info
    cov = landmark_cov.new_zeros(n, 21, 3, 3)
    for k, (a, b) in enumerate(_COV6):
        cov[:, :, a, b] = landmark_cov[:, :, k]
        cov[:, :, b, a] = landmark_cov[:, :, k]
    sigma = torch.sqrt(landmark_cov[:, :, 0] + landmark_cov[:, :, 2] + landmark_cov[:, :, 5])
    out = (h.reshape(lead + (26, 26)), pivot.reshape(lead + (3,)), param_sigma.reshape(lead + (26,)), cov.reshape(lead + (21, 3, 3)),
           sigma.reshape(lead + (21,)), info[:, 3].to(torch.int64).reshape(lead))
    return PoseUncertainty(*(t if device is None else t.to(device) for t in out))


def angle_sigma_from_limits(hand_model: HandModel) -> torch.Tensor:
    """[...,20] (hi - lo) / sqrt(12) of hand_model.joint_limits: the sigma of a uniform law over each angle's box, what
    pose_uncertainty_views takes as `angle_sigma` when nothing better is known about an angle."""
    if hand_model.joint_limits is None:
        raise ValueError("angle_sigma_from_limits needs hand_model.joint_limits")
    box = hand_model.joint_limits[..., :20, :].to(torch.float32)
    return (box[..., 1] - box[..., 0]) / float(np.sqrt(12.0))


def pose_uncertainty_views(hand_model: HandModel, joint_angles: torch.Tensor, wrist_transforms: torch.Tensor, window: torch.Tensor,
                           cam_rows: torch.Tensor, table: torch.Tensor, weights: Optional[torch.Tensor] = None,
                           angle_sigma: Optional[torch.Tensor] = None, loss="squared", loss_scale: float = 3.0,
                           mirror: Optional[torch.Tensor] = None) -> PoseUncertainty:
    """How well the pose (joint_angles [...,22], wrist_transforms [...,4,4]) is known from the detections fit_landmarks_views
    fitted it to, on the HIP kernel csrc/pose_info_views.hip (no CPU implementation): window, cam_rows, table, weights, loss,
    loss_scale and mirror as there, evaluated at the pose as given - one launch, nothing is fitted.  weights are informations:
    with 1 / sigma^2 of each detection in px^-2 the result is absolute, with None it is per px^2 of detection noise.
    angle_sigma [...,20] or [20] rad: a Gaussian prior on each joint angle (angle_sigma_from_limits), the whole answer for an
    angle no used detection depends on, negligible for the others; without it such a pose is COV_SINGULAR and its sigmas are
    +inf.  The covariance is the Gauss-Newton one of the unconstrained linearisation (no second-order term; under a robust loss
    that of the reweighted problem): it means something at a minimum of the cost - at the pose a fit returned.  A hand that
    one camera sees comes back several times less certain along that camera's rays than across them."""
    s, _v, views, weights = _views_staging(hand_model, window, cam_rows, table, weights, False)
    if angle_sigma is not None:
        rows = s.blob.shape[0]
        angle_sigma = torch.as_tensor(angle_sigma, dtype=torch.float32)      # one row per model row, as the kernel reads it
        angle_sigma = angle_sigma.reshape(1, 20) if angle_sigma.numel() == 20 and rows == 1 else angle_sigma.expand(s.lead + (20,)).reshape(s.n, 20)
        if angle_sigma.shape[0] != rows:
            raise ValueError("angle_sigma must be [20] with an unbatched hand_model")
        angle_sigma = angle_sigma.to(s.dev).contiguous()
    outs = _native.pose_information_views(s.blob, s.f32(joint_angles, (22,)), s.f32(wrist_transforms, (4, 4)), *views, weights,
                                          angle_sigma, s.flags(mirror), loss=loss, loss_scale=loss_scale)
    return unpack_uncertainty(*outs, lead=s.lead, device=s.src_device)


SMOOTH_OK, SMOOTH_SINGULAR, SMOOTH_REFUSED, SMOOTH_GAP = (_native.UT_SMOOTH_OK, _native.UT_SMOOTH_SINGULAR, _native.UT_SMOOTH_REFUSED,
                                                            _native.UT_SMOOTH_GAP)


def step_sigma_from_rates(angle_rate: float, rotation_rate: float, speed: float, fps: float) -> torch.Tensor:
    """[26] step_sigma of smooth_poses from what a hand does per second: the joint angles' rate (rad / s), the wrist's turning
    rate (rad / s) and the hand's speed (landmark units / s), each as a standard deviation, at `fps` frames per second.  A random
    walk: the sigma of one frame step is the rate over fps."""
    if not fps > 0:
        raise ValueError("fps must be positive")
    return torch.tensor([angle_rate / fps] * 20 + [rotation_rate / fps] * 3 + [speed / fps] * 3, dtype=torch.float32)


def smooth_poses(hand_model: HandModel, joint_angles: torch.Tensor, wrist_transforms: torch.Tensor, uncertainty, step_sigma,
                 frame_weight: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
                 mirror: Optional[torch.Tensor] = None, centre: Optional[torch.Tensor] = None, return_sigma: bool = False):
    """A sequence of fitted poses smoothed by their information matrices, on the HIP kernel csrc/smooth.hip (no CPU
    implementation): joint_angles [...,T,22] and wrist_transforms [...,T,4,4] are the fits of T consecutive frames, `uncertainty`
    their PoseUncertainty (pose_uncertainty_views; leading dims [...,T]) or the pair (pose_info [...,T,26,26] or packed
    [...,T,351], pivot [...,T,3]).  Every fit is a Gaussian measurement of the true pose, consecutive poses differ by a random
    walk with the standard deviations step_sigma [26] or [...,26] per frame step (20 angles rad, rotation rad, translation in the
    landmarks' units: step_sigma_from_rates), and the result is the most probable sequence - one linear solve, first order in
    the rotation (include/umetrack_hip_smooth.h).  frame_weight [...,T] >= 0 multiplies a frame's information: 0 makes the frame
    a gap that the motion model fills in, as a refused fit (information 0) is.  lengths [...] i32: frames at or past a
    sequence's length are copied through.  centre [...,3] or [3]: the body-fixed point whose motion step_sigma's translation
    describes, in the wrist's frame; default the mean of hand_model.landmark_rest_positions (mirror [...] of 0 / 1: x negated
    where 1, as the landmarks of a mirrored hand are).  Returns (joint_angles, wrist_transforms, info [...,T,4]: how many of its
    own sigmas the frame was moved, the smoothed step in step sigmas, the smallest scaled pivot, status SMOOTH_OK (| SMOOTH_GAP) /
    SMOOTH_SINGULAR (no frame observes some direction: poses unchanged) / SMOOTH_REFUSED) and, with return_sigma=True, param_sigma
    [...,T,26] of the smoothed poses - its translation is that of `centre`."""
    if joint_angles.dim() < 2 or joint_angles.shape[-1] != 22:
        raise ValueError(f"joint_angles must be [...,T,22], got {tuple(joint_angles.shape)}")
    lead, frames = tuple(joint_angles.shape[:-2]), joint_angles.shape[-2]
    src = joint_angles.device
    dev = src if src.type == "cuda" else fk_device()
    n_seq = int(np.prod(lead)) if lead else 1
    pose_info, pivot = (uncertainty.pose_info, uncertainty.pivot) if isinstance(uncertainty, PoseUncertainty) else uncertainty
    if pose_info.shape[-1] == 26 and pose_info.dim() >= 2 and pose_info.shape[-2] == 26:
        pose_info = pose_info[..., _TRIL[0], _TRIL[1]]
    put = lambda t, tail, dtype=torch.float32: None if t is None else torch.as_tensor(t).expand(lead + tail).reshape((n_seq,) + tail).to(dev, dtype).contiguous()
    step_var = torch.as_tensor(step_sigma, dtype=torch.float32)
    step_var = (step_var * step_var).reshape(1, 26) if step_var.numel() == 26 else put(step_var * step_var, (26,))
    if centre is None:
        centre = torch.as_tensor(hand_model.landmark_rest_positions).reshape(-1, 21, 3)[0].to(torch.float64).mean(0).to(torch.float32)
        centre = centre.expand(lead + (3,)).clone()
        if mirror is not None:
            centre[..., 0] = torch.where(torch.as_tensor(mirror).expand(lead) == 1, -centre[..., 0], centre[..., 0])
    ja, xf, sigma, info = _native.smooth_pose_sequence(
        put(joint_angles, (frames, 22)), put(wrist_transforms, (frames, 4, 4)), put(pose_info, (frames, 351)), put(pivot, (frames, 3)),
        step_var.to(dev), put(frame_weight, (frames,)), put(lengths, (), torch.int32), put(centre, (3,)), param_sigma=bool(return_sigma))
    back = lambda t, tail: t.reshape(lead + (frames,) + tail).to(src)
    out = (back(ja, (22,)), back(xf, (4, 4)), back(info, (4,)))
    return out + ((back(sigma, (26,)),) if return_sigma else ())


FITS_CONVERGED, FITS_AT_MAX_ITERS, FITS_REFUSED, FITS_AT_BOUND = (_native.UT_FITS_CONVERGED, _native.UT_FITS_AT_MAX_ITERS,
                                                                  _native.UT_FITS_REFUSED, _native.UT_FITS_AT_BOUND)


def _scale_fit_inputs(hand_model: HandModel, landmarks, weights, init, init_scale, limits, mirror):
    """What fit_landmarks_scale and calibrate_scale hand to _native.fit_pose_scale, flattened to n poses on the device."""
    s = _FitStaging(hand_model, tuple(landmarks.shape[:-2]), landmarks.device, limits, broadcast=True)
    ja, xf = s.init(init)
    return s, dict(hand_model=s.blob, targets=s.f32(landmarks, (21, 3)), weights=s.f32(weights, (21,)), limits=s.box,
                   init_scale=s.f32(init_scale, ()), init_angles=ja, init_wrist_xf=xf, mirror=s.flags(mirror))


def fit_landmarks_scale(hand_model: HandModel, landmarks: torch.Tensor, weights: Optional[torch.Tensor] = None, init=None,
                        init_scale=None, fixed: bool = False, limits: bool = False, mirror: Optional[torch.Tensor] = None,
                        max_iters: int = 32):
    """fit_landmarks with the hand's scale as a parameter, on the HIP kernel csrc/fit_scale.hip (no CPU implementation):
    [...,21,3] landmarks -> (joint_angles [...,22], wrist_transforms [...,4,4], scale [...], info [...,6]) with
    skin_landmarks(scaled_hand_model(hand_model, scale), joint_angles, wrist_transforms) ~ landmarks.  init_scale [...] (or a
    number) is where the scale starts, 1 by default; fixed=True keeps it there, which fits the poses of a calibrated model
    without building it.  info: weighted rms residual, worst residual, iterations, status - FITS_CONVERGED |
    FITS_AT_MAX_ITERS | FITS_REFUSED | FITS_AT_BOUND -, scale information (1 / variance of ln scale per unit^2 of landmark
    noise; 0 with fixed=True), 0.  Everything else as for fit_landmarks."""
    s, args = _scale_fit_inputs(hand_model, landmarks, weights, init, init_scale, limits, mirror)
    ja, xf, scale, info = _native.fit_pose_scale(scale_mode=_native.UT_SCALE_FIXED if fixed else _native.UT_SCALE_FREE,
                                                 max_iters=max_iters, **args)
    return s.back(ja, (22,)), s.back(xf, (4, 4)), s.back(scale, ()), s.back(info, (6,))


class ScaleCalibration(NamedTuple):
    """What calibrate_scale returns.  scale [...]: one per group; stats [...,4]: the scale again, sigma - the standard
    deviation of ln scale per unit of landmark noise -, scatter - the landmark noise that would explain how much the poses
    disagree -, poses used; hand_model: scaled_hand_model(hand_model, scale) when there is one group and the model is
    unbatched, else None; joint_angles [...,N,22], wrist_transforms [...,N,4,4], info [...,N,6]: the poses refitted at the
    calibrated scale (refit=True), else those of the free pass with their own scales in pose_scale [...,N]."""
    scale: torch.Tensor
    stats: torch.Tensor
    hand_model: Optional[HandModel]
    joint_angles: torch.Tensor
    wrist_transforms: torch.Tensor
    info: torch.Tensor
    pose_scale: torch.Tensor


def calibrate_scale(hand_model: HandModel, landmarks: torch.Tensor, weights: Optional[torch.Tensor] = None,
                    mirror: Optional[torch.Tensor] = None, refit: bool = True, max_iters: int = 32) -> ScaleCalibration:
    """One scale for each group of N poses of one person: landmarks [...,N,21,3] (weights [...,N,21], mirror [...,N]) ->
    ScaleCalibration.  A free pass of fit_landmarks_scale over all poses, the information-weighted pool over the N axis
    (ut_pool_scale: poses that did not converge, were refused or ended at a scale bound do not count), and with refit=True
    a second pass at the pooled scale, warm-started from the first.  Three launches, no host work in between.  ValueError
    when a group has no usable pose."""
    if landmarks.dim() < 3:
        raise ValueError(f"landmarks must be [...,N,21,3], got {tuple(landmarks.shape)}")
    s, args = _scale_fit_inputs(hand_model, landmarks, weights, None, None, False, mirror)

    def fixed_pass(ja, xf, pose_scale):
        return _native.fit_pose_scale(scale_mode=_native.UT_SCALE_FIXED, max_iters=max_iters,
                                      **dict(args, init_scale=pose_scale, init_angles=ja, init_wrist_xf=xf))
    return _pooled_calibration(hand_model, s, _native.fit_pose_scale(max_iters=max_iters, **args), fixed_pass, refit, "calibrate_scale")


def _pooled_calibration(hand_model: HandModel, s: _FitStaging, free, fixed_pass, refit: bool, who: str) -> ScaleCalibration:
    """The tail calibrate_scale and calibrate_scale_in_views share: free = (joint_angles, wrist_xf, scale, info) of the free pass
    over s.n poses, pooled over the last leading dim; with refit, fixed_pass(joint_angles, wrist_xf, pose_scale) runs the fixed
    pass from them at the pooled scales; `who` names the caller when a group has no usable pose."""
    ja, xf, scale, info = free
    group_lead, n_per = s.lead[:-1], s.lead[-1]
    group, pose_scale = _native.pool_scale(scale, info, n_per)
    if refit:
        ja, xf, pose_scale, info = fixed_pass(ja, xf, pose_scale)
    else:
        pose_scale = scale
    stats = group.reshape(group_lead + (4,)).to(s.src_device)
    if bool((stats[..., 3] == 0).any()):
        raise ValueError(f"{who}: a group has no usable pose (none converged away from the scale bounds)")
    pooled = stats[..., 0]
    model = None
    if group_lead == () and hand_model.joint_rest_positions.dim() == 2:
        model = scaled_hand_model(hand_model, float(pooled))
    return ScaleCalibration(pooled, stats, model, s.back(ja, (22,)), s.back(xf, (4, 4)), s.back(info, (6,)), s.back(pose_scale, ()))


def _views_scale_inputs(hand_model: HandModel, window, cam_rows, table, init, init_scale, weights, mirror, limits, who):
    """What fit_landmarks_views_scale and calibrate_scale_in_views hand to _native.fit_pose_views_scale, flattened to n poses on
    the device: (staging, V, positional arguments, keyword arguments)."""
    if init is None:
        raise ValueError(f"init = (joint_angles, wrist_transforms) is required: {who} has no cold start")
    s, v, views, weights = _views_staging(hand_model, window, cam_rows, table, weights, limits)
    if init_scale is not None:
        init_scale = torch.as_tensor(init_scale).expand(s.lead)
    return s, v, (s.blob, *views, *s.init(init)), dict(weights=weights, limits=s.box, init_scale=s.f32(init_scale, ()), mirror=s.flags(mirror))


def fit_landmarks_views_scale(hand_model: HandModel, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor, init,
                              init_scale=None, fixed: bool = False, weights: Optional[torch.Tensor] = None,
                              mirror: Optional[torch.Tensor] = None, limits=None, max_iters: int = 32, with_residual: bool = False,
                              loss="squared", loss_scale: float = 3.0, return_inliers: bool = False):
    """fit_landmarks_views with the hand's scale as a parameter, on the HIP kernel csrc/fit_views_scale.hip (no CPU
    implementation): the pose AND the scale whose landmarks, projected into the views, meet the detections.  Returns
    (joint_angles [...,22], wrist_transforms [...,4,4], scale [...], info [...,6]: rms px of the (robust) cost, largest raw
    reprojection distance px, iterations, status - FITS_CONVERGED | FITS_AT_MAX_ITERS | FITS_REFUSED | FITS_AT_BOUND -, scale
    information (1 / variance of ln scale per px^2 of detection noise; 0 with fixed=True), 0) and then, as for
    fit_landmarks_views, the reprojection distances (with_residual=True) and psi of every used detection (return_inliers=True).
    init_scale [...] (or a number) is where the scale starts, 1 by default; fixed=True keeps it there, which fits the poses of a
    calibrated model without building it.  One camera cannot see the hand's size: with one view a free fit returns a scale that
    means nothing and an information near 0 - use fixed=True on one-view frames.  window, cam_rows, table, init (required),
    weights, mirror, limits, loss and loss_scale as for fit_landmarks_views."""
    s, v, args, kw = _views_scale_inputs(hand_model, window, cam_rows, table, init, init_scale, weights, mirror, limits,
                                         "fit_landmarks_views_scale")
    res = _native.fit_pose_views_scale(*args, scale_mode=_native.UT_SCALE_FIXED if fixed else _native.UT_SCALE_FREE, max_iters=max_iters,
                                       loss=loss, loss_scale=loss_scale, residual=with_residual, inlier=return_inliers, **kw)
    out = (s.back(res[0], (22,)), s.back(res[1], (4, 4)), s.back(res[2], ()), s.back(res[3], (6,)))
    return out + tuple(s.back(r, (v, 21)) for r in res[4:])


def calibrate_scale_in_views(hand_model: HandModel, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor, init,
                             init_scale=None, weights: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None,
                             refit: bool = True, loss="squared", loss_scale: float = 3.0, max_iters: int = 32) -> ScaleCalibration:
    """calibrate_scale on the detections themselves: one scale for each group of N poses of one person from window
    [...,N,V,21,2], cam_rows [...,N,V] and table as for fit_landmarks_views (weights [...,N,V,21], mirror [...,N]) ->
    ScaleCalibration, whose sigma and scatter are per px of detection noise.  init = (joint_angles [...,N,22], wrist_transforms
    [...,N,4,4]) and init_scale [...,N] (or a number; 1 by default) are the start - the 3-D chain's free pass, e.g.
    calibrate_scale(..., refit=False).  A free pass of fit_landmarks_views_scale over all poses, the information-weighted pool
    over the N axis (ut_pool_scale: poses that did not converge, were refused or ended at a scale bound do not count, and a pose
    one camera alone sees carries next to no information), and with refit=True a fixed pass at the pooled scale, warm-started
    from the first.  Three launches, no host work in between.  loss, loss_scale: both passes'.  ValueError when a group has no
    usable pose."""
    if window.dim() < 4:
        raise ValueError(f"window must be [...,N,V,21,2], got {tuple(window.shape)}")
    s, _v, args, kw = _views_scale_inputs(hand_model, window, cam_rows, table, init, init_scale, weights, mirror, None,
                                          "calibrate_scale_in_views")
    kw.update(max_iters=max_iters, loss=loss, loss_scale=loss_scale)

    def fixed_pass(ja, xf, pose_scale):
        return _native.fit_pose_views_scale(*args[:4], ja, xf, scale_mode=_native.UT_SCALE_FIXED, **dict(kw, init_scale=pose_scale))
    return _pooled_calibration(hand_model, s, _native.fit_pose_views_scale(*args, **kw), fixed_pass, refit, "calibrate_scale_in_views")


_MESH_FIELDS = ("mesh_vertices", "mesh_triangles", "dense_bone_weights")
_mesh_cache: list = []      # [(key, tensors kept alive, _native.Mesh)], most recent first


def _mesh_tensors(hand_model: HandModel) -> tuple:
    tensors = tuple(getattr(hand_model, f) for f in _MESH_FIELDS)
    if any(t is None for t in tensors):
        raise ValueError("the hand model carries no mesh (mesh_vertices, mesh_triangles and dense_bone_weights are needed)")
    if any(t.dim() != 2 for t in tensors):
        raise ValueError("mesh fields must be unbatched ([V,3], [T,3], [V,17]); got "
                         + ", ".join(str(tuple(t.shape)) for t in tensors))
    return tensors


def device_mesh(hand_model: HandModel, dev: torch.device) -> "_native.Mesh":
    """The model's mesh packed for csrc/mesh.hip (sparse weights, vertex -> triangle table) and resident on `dev`, cached
    like device_blob: keyed on tensor identity + in-place version counters.  ValueError for a model without a mesh, for
    batched mesh fields (one mesh per launch) and for a mesh the library refuses."""
    tensors = _mesh_tensors(hand_model)
    dev = torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (str(dev),) + tuple((id(t), t._version) for t in tensors)
    for i, (k, _keep, mesh) in enumerate(_mesh_cache):
        if k == key:
            if i:
                _mesh_cache.insert(0, _mesh_cache.pop(i))
            return mesh
    mesh = _native.Mesh(*tensors, device=dev)
    _mesh_cache.insert(0, (key, tensors, mesh))
    del _mesh_cache[8:]
    return mesh


def skin_mesh(hand_model: HandModel, joint_angles: torch.Tensor, wrist_transforms: torch.Tensor, normals: bool = False,
              mirror: Optional[torch.Tensor] = None):
    """[...,22] joint angles + [...,4,4] wrist transforms -> the posed mesh [...,V,3], or (vertices, unit normals) with
    normals=True: the reference's _skin_points (lib/common/hand_skinning.py:154-186) on mesh_vertices /
    dense_bone_weights, on the HIP kernel csrc/mesh.hip (no CPU implementation).  Leading dims as for skin_landmarks;
    the skeleton fields are unbatched or carry them, the mesh fields are unbatched.  mirror (optional, [...] of 0 / 1):
    where 1, column 0 of the wrist transform is negated on the device - the right-hand convention of
    lib/tracker/perspective_crop.py:48-49 - and the normals are kept pointing outwards."""
    lead = tuple(joint_angles.shape[:-1])
    n = int(np.prod(lead)) if lead else 1
    model_lead = tuple(hand_model.joint_rest_positions.shape[:-2])
    if model_lead not in ((), lead):
        raise AssertionError(f"Leading dimensions do not match, got {lead} and {model_lead}")
    _mesh_tensors(hand_model)                    # a model without a usable mesh is refused before a device is needed
    src_device = joint_angles.device
    dev = src_device if src_device.type == "cuda" else fk_device()
    res = _native.skin_mesh(device_mesh(hand_model, dev), device_blob(hand_model, dev),
                            joint_angles.reshape(n, 22).to(dev, torch.float32),
                            wrist_transforms.reshape(n, 4, 4).to(dev, torch.float32),
                            mirror=None if mirror is None else mirror.reshape(n).to(dev, torch.int64), normals=normals)
    shape = lead + (hand_model.mesh_vertices.shape[0], 3)
    if normals:
        return res[0].reshape(shape).to(src_device), res[1].reshape(shape).to(src_device)
    return res.reshape(shape).to(src_device)


def render_mesh(hand_model: HandModel, joint_angles: torch.Tensor, wrist_transforms: torch.Tensor, crop_cameras,
                mirror: Optional[torch.Tensor] = None, sample_range: Optional[torch.Tensor] = None):
    """Pose the model's mesh (skin_mesh) and rasterise it into 96x96 pinhole crop cameras on the HIP kernel csrc/render.hip
    (no CPU implementation): (depth f32 [N,96,96] eye-space z of the nearest surface, +inf on background; tri i32 [N,96,96]
    the triangle seen, -1 on background; shade u8 [N,96,96] flat headlight shading, 0 on background).
    joint_angles [n,22] (or [22]), wrist_transforms [n,4,4], mirror as for skin_mesh.  crop_cameras: an f64 [N,24] tensor /
    array of crop_params rows (geometry.pack_crop_camera), or a list of PinholePlaneCameraModel.  sample_range i64 [n,2]:
    pose i is drawn into crops [sample_range[i,0], sample_range[i,1]) - at most two; by default every pose is drawn into
    N / n consecutive crops.  Results come back on the device of joint_angles."""
    from . import geometry
    ja = joint_angles.reshape(-1, 22)
    n = ja.shape[0]
    src_device = joint_angles.device
    dev = src_device if src_device.type == "cuda" else fk_device()
    if isinstance(crop_cameras, (list, tuple)):
        crop_cameras = np.stack([geometry.pack_camera_model(c) for c in crop_cameras]) if len(crop_cameras) else np.zeros((0, 24))
    if not isinstance(crop_cameras, torch.Tensor):
        crop_cameras = torch.from_numpy(np.ascontiguousarray(crop_cameras, np.float64))
    crop_params = crop_cameras.reshape(-1, 24).to(dev, torch.float64)
    if sample_range is None:
        per = crop_params.shape[0] // max(n, 1)
        if per * n != crop_params.shape[0] or per > 2:
            raise ValueError(f"{crop_params.shape[0]} crop cameras for {n} poses: give sample_range")
        ends = torch.arange(1, n + 1, dtype=torch.int64) * per
        sample_range = torch.stack([ends - per, ends], 1)
    mesh = device_mesh(hand_model, dev)
    verts = _native.skin_mesh(mesh, device_blob(hand_model, dev), ja.to(dev, torch.float32),
                              wrist_transforms.reshape(n, 4, 4).to(dev, torch.float32),
                              mirror=None if mirror is None else mirror.reshape(n).to(dev, torch.int64))
    depth, tri, shade = _native.render_mesh(mesh, verts, crop_params, sample_range.to(dev, torch.int64))
    return depth.to(src_device), tri.to(src_device), shade.to(src_device)


def overlay(crops: torch.Tensor, shade: torch.Tensor, tri: torch.Tensor, alpha: float = 0.6) -> torch.Tensor:
    """The shaded hand laid over fp32 crops [N,96,96] (HotPath(keep_crops=True).crops): where a triangle is seen
    (tri >= 0) the pixel becomes (1 - alpha) * crop + alpha * shade / 255 * (the crops' largest value), elsewhere it stays.
    Plain torch on the tensors' device; no kernel."""
    white = crops.max().clamp_min(1e-12) if crops.numel() else crops.new_ones(())
    lit = shade.to(crops.dtype) * (white / 255.0)
    return torch.where(tri >= 0, (1.0 - alpha) * crops + alpha * lit, crops)
