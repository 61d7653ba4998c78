"""ctypes binding of libumetrack_hip.so (include/umetrack_hip.h and its extension headers include/umetrack_hip_fit.h,
include/umetrack_hip_triangulate.h, include/umetrack_hip_scale.h, include/umetrack_hip_info.h, include/umetrack_hip_views.h,
include/umetrack_hip_robust.h, include/umetrack_hip_views_scale.h and include/umetrack_hip_uncertainty.h).

There is no CPU fallback: if the shared library is missing or no HIP device is
present, every entry point raises.  PyTorch-ROCm is used for device memory and
streams only; tensors cross the boundary as raw device pointers.
"""
import contextlib
import ctypes
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import arch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libumetrack_hip.so")

_vp, _i32, _f32, _f64, _sz, _P = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                                  ctypes.POINTER)
# Every entry of include/umetrack_hip.h, in the header's order: name -> (restype, argtypes).  load_library() declares
# exactly these, so an entry cannot be exported without its prototype (tests compare the counts with the header).
_PROTOTYPES = {
    "ut_weight_blob_floats": (_sz, []),
    "ut_create": (_i32, [_i32, _vp, _sz, _P(_vp)]),
    "ut_canonical_backbone_weights": (_i32, [_vp, _sz, _vp, _sz, _P(_sz)]),
    "ut_destroy": (_i32, [_vp]),
    "ut_last_error": (ctypes.c_char_p, [_vp]),
    "ut_set_index_checks": (_i32, [_vp, _i32]),
    "ut_poll_status": (_i32, [_vp, _vp]),
    "ut_status_snapshot": (_i32, [_vp, _vp, _vp]),
    "ut_set_backbone_lanes": (_i32, [_vp, _i32]),
    "ut_set_conv_arithmetic": (_i32, [_vp, _i32]),
    "ut_set_split_scale": (_i32, [_vp, _i32]),
    "ut_get_split_adaptations": (_i32, [_vp, _P(ctypes.c_uint32), _i32, _vp]),
    "ut_calibrate_split": (_i32, [_vp, _vp, _i32, _vp]),
    "ut_get_split_calibration": (_i32, [_vp, _vp]),
    "ut_set_block_fusion": (_i32, [_vp, _i32]),
    "ut_set_resident_weights": (_i32, [_vp, _i32]),
    "ut_set_latency_mode": (_i32, [_vp, _i32]),
    "ut_reserve": (_i32, [_vp, _i32, _i32, _i32]),
    "ut_set_backbone_chunk": (_i32, [_vp, _i32]),
    "ut_warp_crops": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "ut_warp_map": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "ut_backbone": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "ut_warp_backbone": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "ut_fuse_temporal_regress": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32,
                                        _vp, _vp, _vp]),
    "ut_reset_memory": (_i32, [_vp]),
    "ut_get_memory": (_i32, [_vp, _vp, _vp, _i32, _vp]),
    "ut_fk": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _vp, _vp]),
    "ut_mesh_create": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _P(_vp)]),
    "ut_mesh_destroy": (_i32, [_vp]),
    "ut_mesh_counts": (_i32, [_vp, _P(_i32), _P(_i32)]),
    "ut_skin_mesh": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _vp, _vp, _vp]),
    "ut_project_points": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ut_render_mesh": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ut_gen_crop_cameras": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                   _i32, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ut_gen_crop_cameras_from_window_points": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _f64, _vp, _vp, _vp,
                                                      _vp, _vp, _vp, _vp]),
    "ut_gen_crop_matrices": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f64, _vp, _vp, _vp, _vp, _vp]),
    "ut_resample_homography": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "ut_keypoint_metrics": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ut_profile_begin": (_i32, [_vp, _vp]),
    "ut_profile_end": (_i32, [_vp, _vp, _P(_f64), _P(ctypes.c_int64), _P(_f64)]),
    "ut_profile_end_by_kind": (_i32, [_vp, _vp, _P(_f64), _P(ctypes.c_int64), _P(_f64)]),
}
EXPORTS = tuple(_PROTOTYPES)
# The entries of the extension headers (include/umetrack_hip_fit.h): umetrack_hip.h's list is closed, later entries have a
# header and a table of their own.  load_library() declares these as well.
_EXTENSION_PROTOTYPES = {
    "ut_fit_pose": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _i32, _vp, _i32, _vp, _i32,
                           _vp, _vp]),
}
EXTENSION_EXPORTS = tuple(_EXTENSION_PROTOTYPES)
# The entry of include/umetrack_hip_triangulate.h, in a table of its own like its header (tests/test_triangulate_host.py pins it).
_TRIANGULATE_PROTOTYPES = {
    "ut_triangulate_points": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
}
TRIANGULATE_EXPORTS = tuple(_TRIANGULATE_PROTOTYPES)
# The entries of include/umetrack_hip_scale.h, in a table of their own like their header (tests/test_scale_host.py pins it).
_SCALE_PROTOTYPES = {
    "ut_fit_pose_scale": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _i32, _vp,
                                 _i32, _vp, _i32, _vp, _vp, _vp]),
    "ut_pool_scale": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
}
SCALE_EXPORTS = tuple(_SCALE_PROTOTYPES)
# The entries of include/umetrack_hip_info.h, in a table of their own like their header (tests/test_info_host.py pins it).
_INFO_PROTOTYPES = {
    "ut_triangulate_points_info": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp,
                                          _vp]),
    "ut_fit_pose_info": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _i32, _vp, _i32, _vp,
                                _i32, _vp, _vp]),
}
INFO_EXPORTS = tuple(_INFO_PROTOTYPES)
# The entry of include/umetrack_hip_views.h, in a table of its own like its header (tests/test_views_host.py pins it).
_VIEWS_PROTOTYPES = {
    "ut_fit_pose_views": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _f32, _i32,
                                 _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
}
VIEWS_EXPORTS = tuple(_VIEWS_PROTOTYPES)
# The entry of include/umetrack_hip_robust.h, in a table of its own like its header (tests/test_robust_host.py pins it).
_ROBUST_PROTOTYPES = {
    "ut_fit_pose_views_robust": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _f32,
                                        _i32, _i32, _f32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
}
ROBUST_EXPORTS = tuple(_ROBUST_PROTOTYPES)
# The entry of include/umetrack_hip_views_scale.h, in a table of its own like its header (tests/test_views_scale_host.py pins it).
_VIEWS_SCALE_PROTOTYPES = {
    "ut_fit_pose_views_scale": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp,
                                       _f32, _i32, _i32, _f32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
}
VIEWS_SCALE_EXPORTS = tuple(_VIEWS_SCALE_PROTOTYPES)
# The entry of include/umetrack_hip_uncertainty.h, in a table of its own like its header (tests/test_uncertainty_host.py pins it).
_UNCERTAINTY_PROTOTYPES = {
    "ut_pose_information_views": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _f32,
                                         _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
}
UNCERTAINTY_EXPORTS = tuple(_UNCERTAINTY_PROTOTYPES)
# The entry of include/umetrack_hip_smooth.h, in a table of its own like its header (tests/test_smooth_host.py pins it).
_SMOOTH_PROTOTYPES = {
    "ut_smooth_pose_sequence": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _i32, _vp, _vp, _i32,
                                       _vp, _i32, _vp, _vp, _vp]),
}
SMOOTH_EXPORTS = tuple(_SMOOTH_PROTOTYPES)
# The entries of include/umetrack_hip_start.h, in a table of their own like their header (tests/test_start_host.py pins it).
_START_PROTOTYPES = {
    "ut_start_pose_views": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _i32,
                                   _vp, _i32, _vp, _i32, _vp, _vp]),
    "ut_select_pose": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
}
START_EXPORTS = tuple(_START_PROTOTYPES)
# The entry of include/umetrack_hip_track.h, in a table of its own like its header (tests/test_track_host.py pins it).
_TRACK_PROTOTYPES = {
    "ut_track_pose_views": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp,
                                   _vp, _f64, _f64, _vp, _vp, _f32, _i32, _i32, _f32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
}
TRACK_EXPORTS = tuple(_TRACK_PROTOTYPES)

UT_MODE_KNOWN, UT_MODE_UNKNOWN = 0, 1
UT_REMAP_CV2_FIXED, UT_REMAP_FLOAT = 0, 1
UT_CHECK_SYNC, UT_CHECK_DEFERRED = 0, 1
SPLIT_SCALE_MODES = {"calibrated": 0, "dynamic": 1, "adaptive": 2}      # UT_SPLIT_SCALE_*

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def load_library() -> ctypes.CDLL:
    """dlopen the in-tree library and declare the prototypes.  Raises loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**_PROTOTYPES, **_EXTENSION_PROTOTYPES, **_TRIANGULATE_PROTOTYPES, **_SCALE_PROTOTYPES,
                                      **_INFO_PROTOTYPES, **_VIEWS_PROTOTYPES, **_ROBUST_PROTOTYPES,
                                      **_VIEWS_SCALE_PROTOTYPES, **_UNCERTAINTY_PROTOTYPES, **_SMOOTH_PROTOTYPES,
                                      **_START_PROTOTYPES, **_TRACK_PROTOTYPES}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def state_dict_to_blob(state_dict) -> np.ndarray:
    """Flatten a reference-keyed state dict (torch tensors or numpy arrays) in the order of
    arch.state_dict_spec() to the fp32 blob ut_create expects.  Strict like load_state_dict."""
    spec = arch.state_dict_spec()
    missing = [k for k, _s, _kind in spec if k not in state_dict]
    extra = [k for k in state_dict if k not in {k for k, _s, _kind in spec}]
    if missing or extra:
        raise RuntimeError(f"Error(s) in loading state_dict: missing keys {missing[:4]}..., "
                           f"unexpected keys {extra[:4]}..." if missing or extra else "")
    parts = []
    for k, shape, _kind in spec:
        v = state_dict[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        if tuple(v.shape) != tuple(shape):
            raise RuntimeError(f"size mismatch for {k}: expected {tuple(shape)}, got {tuple(v.shape)}")
        parts.append(v.astype(np.float32).reshape(-1))
    blob = np.ascontiguousarray(np.concatenate(parts))
    assert blob.size == 4_259_410
    return blob


def canonical_backbone_weights(state_dict) -> np.ndarray:
    """The backbone's folded convolutions at their canonical channel scales, as ut_create packs them (host only: runs
    without a GPU).  Layout: see ut_canonical_backbone_weights in include/umetrack_hip.h."""
    lib = load_library()
    blob = state_dict_to_blob(state_dict)
    n = ctypes.c_size_t()
    rc = lib.ut_canonical_backbone_weights(blob.ctypes.data_as(ctypes.c_void_p), blob.size, None, 0, ctypes.byref(n))
    _check_rc(lib, None, rc, "ut_canonical_backbone_weights")
    out = np.empty(n.value, np.float32)
    rc = lib.ut_canonical_backbone_weights(blob.ctypes.data_as(ctypes.c_void_p), blob.size,
                                           out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n))
    _check_rc(lib, None, rc, "ut_canonical_backbone_weights")
    return out


def hand_model_blob(joint_rotation_axes, joint_rest_positions, landmark_rest_positions,
                    landmark_rest_bone_weights, landmark_rest_bone_indices) -> np.ndarray:
    """[...,321] fp32 packing of the HandModel fields the FK kernel reads (lib/common/hand.py:48-62)."""
    def a(x, tail):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        x = np.asarray(x, np.float32)
        return x.reshape(x.shape[: x.ndim - len(tail)] + (-1,))
    parts = [a(joint_rotation_axes, (22, 3)), a(joint_rest_positions, (22, 3)), a(landmark_rest_positions, (21, 3)),
             a(landmark_rest_bone_weights, (21, 3)), a(landmark_rest_bone_indices, (21, 3))]
    lead = np.broadcast_shapes(*[p.shape[:-1] for p in parts])
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(p, lead + p.shape[-1:]) for p in parts], -1))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need(t: torch.Tensor, dtype, device, name: str) -> torch.Tensor:
    if t.device != device:
        raise ValueError(f"{name} must live on {device}, got {t.device}")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _hip_device(t: torch.Tensor, who: str) -> torch.device:
    if t.device.type != "cuda":
        raise NativeLibraryError(f"{who} needs tensors on a HIP device (no CPU fallback)")
    return t.device


def _out(t: Optional[torch.Tensor], shape, dtype, device, name: str, fill=None, flat: bool = False) -> torch.Tensor:
    """The output buffer of a call.  t is None: a fresh tensor, filled with `fill` if one is given.  Otherwise the caller's
    own, returned as it is (never pre-filled): it must be contiguous, of this dtype, on this device and of this shape - with
    flat=True of this many elements, so that e.g. a [n,V,9] staging view stands for [n,V,3,3] - else ValueError."""
    shape = tuple(shape)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)
    same = t.numel() == int(np.prod(shape)) if flat else tuple(t.shape) == shape
    if not same or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} {shape} tensor on {device}")
    return t


# How a negative return code becomes an exception, per family of entries: (class of UT_E_INVALID, class of UT_E_UNSUPPORTED,
# {marker in a UT_E_INVALID message: its class}); every other code is a RuntimeError.
_UT_E_INVALID, _UT_E_UNSUPPORTED = -1, -4
_ERROR_CLASSES = {
    # HipEngine methods: the reference asserts where the library says "unsupported" (umetrack_model.py:224-229), its tensor
    # indexing raises IndexError, and the split-fp16 backbone reports an infinity / a NaN among a layer's inputs
    "engine": (RuntimeError, AssertionError, {"index check:": IndexError, "range check:": FloatingPointError}),
    "points": (ValueError, ValueError, {"index check:": IndexError}),        # project_points, render_mesh, triangulate_points
    "mesh": (ValueError, ValueError, {}),                                    # Mesh(...): the library refused the mesh
    "stateless": (RuntimeError, RuntimeError, {}),
}


def _check_rc(lib, h, rc: int, what: str, family: str = "stateless") -> int:
    """Return a non-negative rc (ut_get_memory's slot count); raise for a negative one with ut_last_error's text - the
    handle's when there is a handle, else the NULL slot's - as the class _ERROR_CLASSES gives this family of entries."""
    if rc >= 0:
        return rc
    invalid, unsupported, marked = _ERROR_CLASSES[family]
    msg = lib.ut_last_error(h).decode()
    cls = RuntimeError
    if rc == _UT_E_UNSUPPORTED:
        cls = unsupported
    elif rc == _UT_E_INVALID:
        cls = next((c for marker, c in marked.items() if marker in msg), invalid)
    raise cls(f"{what} failed ({rc}): {msg}")


def _fk_args(d, hand_model, joint_angles, wrist_xf, mirror, n: Optional[int]):
    """The pose arguments of ut_fk / ut_skin_mesh on device d: hand_model [1|n,321]; joint_angles / wrist_xf either packed
    [n,22] / [n,4,4] (n None) or, with n given, fp32 views into a pose-record buffer that are read in place with the
    caller's strides; mirror [n] or None.  Returns them ready for the call, with n."""
    hand_model = _need(hand_model, torch.float32, d, "hand_model").reshape(-1, 321)
    if n is None:
        joint_angles = _need(joint_angles, torch.float32, d, "joint_angles").reshape(-1, 22)
        wrist_xf = _need(wrist_xf, torch.float32, d, "wrist_xf").reshape(-1, 16)
        n = joint_angles.shape[0]
        if wrist_xf.shape[0] != n:
            raise ValueError("joint_angles / wrist_xf batch mismatch")
    elif joint_angles.device != d or wrist_xf.device != d or joint_angles.dtype != torch.float32 or wrist_xf.dtype != torch.float32:
        raise ValueError(f"strided pose views must be fp32 on {d}")
    if hand_model.shape[0] not in (1, n) and n:
        raise ValueError(f"hand_model has {hand_model.shape[0]} rows for {n} poses")
    if mirror is not None:
        mirror = _need(mirror, torch.int64, d, "mirror").reshape(-1)
        if mirror.shape[0] != n:
            raise ValueError("mirror batch mismatch")
    return hand_model, joint_angles, wrist_xf, mirror, n


def _fk(lib, h, d, family, hand_model, joint_angles, wrist_xf, mirror, t_scale, ja_stride=22, xf_stride=16, n=None, out=None):
    """ut_fk with a model handle (HipEngine.fk) or without one (fk_stateless)."""
    hand_model, joint_angles, wrist_xf, mirror, n = _fk_args(d, hand_model, joint_angles, wrist_xf, mirror, n)
    if out is None:
        out = torch.empty(n, arch.N_LANDMARKS, 3, dtype=torch.float32, device=d)
    _check_rc(lib, h, lib.ut_fk(h, _ptr(hand_model), hand_model.shape[0], _ptr(joint_angles), ja_stride, _ptr(wrist_xf),
                                xf_stride, _ptr(mirror), ctypes.c_float(t_scale), n, _ptr(out), _stream(d)), "ut_fk", family)
    return out


def fk_stateless(hand_model: torch.Tensor, joint_angles: torch.Tensor, wrist_xf: torch.Tensor,
                 mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0) -> torch.Tensor:
    """ut_fk without a model handle (the FK kernel needs no network weights).  All tensors on one HIP device."""
    d = _hip_device(joint_angles, "fk_stateless")
    with torch.cuda.device(d):
        return _fk(load_library(), None, d, "stateless", hand_model, joint_angles, wrist_xf, mirror, t_scale)


UT_FIT_CONVERGED, UT_FIT_AT_MAX_ITERS, UT_FIT_REFUSED = 1, 2, 4


def fit_pose(hand_model: torch.Tensor, targets: torch.Tensor, weights: Optional[torch.Tensor] = None,
             limits: Optional[torch.Tensor] = None, init_angles: Optional[torch.Tensor] = None,
             init_wrist_xf: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
             max_iters: int = 32, *, n: Optional[int] = None, target_stride: int = 63, init_ja_stride: int = 22,
             init_xf_stride: int = 16, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_stride: int = 22,
             xf_stride: int = 16, info: Optional[torch.Tensor] = None, engine: Optional["HipEngine"] = None):
    """ut_fit_pose, the inverse of ut_fk: (joint_angles, wrist_xf, info [n,4]: weighted rms residual, worst residual,
    iterations, status bits UT_FIT_*).  hand_model [1|n,321]; targets [n,21,3]; weights [n,21] or None; limits [1|n,20,2] (one
    row per model row) or None; init_angles / init_wrist_xf [n,22] / [n,4,4], both or neither (cold start); mirror [n] or
    None.  Packed tensors by default, outputs fresh [n,22] / [n,4,4].  With n given, targets / init_* / out are fp32 views
    used in place with the strides given in floats - keypoints and poses inside record buffers, `out` may be the init's
    own views.  All tensors on one HIP device; `engine` only lends its handle for error reporting."""
    return _fit_pose("ut_fit_pose", hand_model, targets, weights, limits, init_angles, init_wrist_xf, mirror, t_scale, max_iters,
                     n, target_stride, init_ja_stride, init_xf_stride, out, ja_stride, xf_stride, info, engine)


def fit_pose_info(hand_model: torch.Tensor, targets: torch.Tensor, sqrt_info: torch.Tensor,
                  limits: Optional[torch.Tensor] = None, init_angles: Optional[torch.Tensor] = None,
                  init_wrist_xf: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                  max_iters: int = 32, *, n: Optional[int] = None, target_stride: int = 63, init_ja_stride: int = 22,
                  init_xf_stride: int = 16, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_stride: int = 22,
                  xf_stride: int = 16, info: Optional[torch.Tensor] = None, engine: Optional["HipEngine"] = None):
    """ut_fit_pose_info: fit_pose with every landmark's residual whitened by the factor of its information, sqrt_info f32
    [n,21,6] - (l00, l10, l11, l20, l21, l22) of the lower Cholesky factor, what triangulate_points_info returns - in place
    of the weights; a landmark whose factor is all 0 is not used and its target not read.  Returns (joint_angles, wrist_xf,
    info [n,4]: whitened rms residual, largest Euclidean residual, iterations, status bits UT_FIT_*).  Every other argument
    as for fit_pose.  Without init_angles / init_wrist_xf this is the C entry's cold start, which can end in a local minimum
    on the anisotropic cost: warm-start from fit_pose's result (hand.fit_landmarks_info does)."""
    if sqrt_info is None:
        raise ValueError("sqrt_info is required")
    return _fit_pose("ut_fit_pose_info", hand_model, targets, sqrt_info, limits, init_angles, init_wrist_xf, mirror, t_scale,
                     max_iters, n, target_stride, init_ja_stride, init_xf_stride, out, ja_stride, xf_stride, info, engine)


def _fit_args(d, hand_model, init_angles, init_wrist_xf, n, batch, strided, out, limits, mirror, engine, windows=False):
    """What the four pose fits marshal alike, on device d: hand_model as [1|n,321]; the init pair, both or neither; the packed
    form (n None: n = batch, the init as [n,22] / [n,16], `out` checked or fresh) against the strided form (n given: the views
    `strided`, the init and `out` are fp32 on d and used in place, `out` is required and, with windows=True, n is the windows'
    batch); limits as one [20,2] row per model row; mirror [n]; the engine's handle.  Returns (hand_model, init_angles,
    init_wrist_xf, n, out, limits, mirror, handle)."""
    hand_model = _need(hand_model, torch.float32, d, "hand_model").reshape(-1, 321)
    if (init_angles is None) != (init_wrist_xf is None):
        raise ValueError("init_angles and init_wrist_xf go together")
    if n is None:
        n = batch
        if init_angles is not None:
            init_angles = _need(init_angles, torch.float32, d, "init_angles").reshape(-1, 22)
            init_wrist_xf = _need(init_wrist_xf, torch.float32, d, "init_wrist_xf").reshape(-1, 16)
            if init_angles.shape[0] != n or init_wrist_xf.shape[0] != n:
                raise ValueError("init_angles / init_wrist_xf batch mismatch")
        if out is not None:
            out = (_out(out[0], (n, 22), torch.float32, d, "out[0]"), _out(out[1], (n, 4, 4), torch.float32, d, "out[1]"))
    else:
        views = list(strided) + ([] if init_angles is None else [init_angles, init_wrist_xf]) + list(out or ())
        if (windows and n != batch) or out is None or any(v.device != d or v.dtype != torch.float32 for v in views):
            also = "n the windows' batch, " if windows else ""
            raise ValueError(f"strided views must be fp32 on {d}, {also}and `out` must be given with them")
    if out is None:
        out = (torch.empty(n, 22, dtype=torch.float32, device=d), torch.empty(n, 4, 4, dtype=torch.float32, device=d))
    if hand_model.shape[0] not in (1, n) and n:
        raise ValueError(f"hand_model has {hand_model.shape[0]} rows for {n} poses")
    if limits is not None:
        limits = _need(limits, torch.float32, d, "limits").reshape(-1, 20, 2)
        if limits.shape[0] != hand_model.shape[0]:
            raise ValueError(f"limits has {limits.shape[0]} rows for {hand_model.shape[0]} model rows")
    if mirror is not None:
        mirror = _need(mirror, torch.int64, d, "mirror").reshape(-1)
        if mirror.shape[0] != n:
            raise ValueError("mirror batch mismatch")
    return hand_model, init_angles, init_wrist_xf, n, out, limits, mirror, engine._h if engine is not None else None


def _fit_call(entry, d, h, *args):
    """The C entry of a pose fit on d's current stream; a negative return code raises."""
    lib = load_library()
    with torch.cuda.device(d):
        rc = getattr(lib, entry)(h, *args, _stream(d))
    _check_rc(lib, h, rc, entry, "points")


def _fit_pose(entry, hand_model, targets, weights, limits, init_angles, init_wrist_xf, mirror, t_scale, max_iters, n,
              target_stride, init_ja_stride, init_xf_stride, out, ja_stride, xf_stride, info, engine):
    """fit_pose and fit_pose_info: `weights` is [n,21] for ut_fit_pose, the factors [n,21,6] for ut_fit_pose_info."""
    d = _hip_device(targets, entry[3:])
    if n is None:
        targets = _need(targets, torch.float32, d, "targets").reshape(-1, 63)
    hand_model, init_angles, init_wrist_xf, n, out, limits, mirror, h = _fit_args(
        d, hand_model, init_angles, init_wrist_xf, n, targets.shape[0], [targets], out, limits, mirror, engine)
    if weights is not None:
        name, shape = ("weights", (n, 21)) if entry == "ut_fit_pose" else ("sqrt_info", (n, 21, 6))
        weights = _need(weights, torch.float32, d, name)
        if tuple(weights.shape) != shape:
            raise ValueError(f"{name} must be [{','.join(map(str, shape))}], got {tuple(weights.shape)}")
    info = _out(info, (n, 4), torch.float32, d, "info")
    _fit_call(entry, d, h, _ptr(hand_model), hand_model.shape[0], _ptr(targets), target_stride, _ptr(weights), _ptr(limits),
              _ptr(init_angles), init_ja_stride, _ptr(init_wrist_xf), init_xf_stride, _ptr(mirror), ctypes.c_float(t_scale),
              int(max_iters), n, _ptr(out[0]), ja_stride, _ptr(out[1]), xf_stride, _ptr(info))
    return out[0], out[1], info


UT_SCALE_FREE, UT_SCALE_FIXED = 0, 1
UT_FITS_CONVERGED, UT_FITS_AT_MAX_ITERS, UT_FITS_REFUSED, UT_FITS_AT_BOUND = 1, 2, 4, 8
UT_SCALE_MIN, UT_SCALE_MAX = 0.25, 4.0


def fit_pose_scale(hand_model: torch.Tensor, targets: torch.Tensor, weights: Optional[torch.Tensor] = None,
                   limits: Optional[torch.Tensor] = None, init_scale: Optional[torch.Tensor] = None,
                   scale_mode: int = UT_SCALE_FREE, init_angles: Optional[torch.Tensor] = None,
                   init_wrist_xf: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                   max_iters: int = 32, *, n: Optional[int] = None, target_stride: int = 63, init_ja_stride: int = 22,
                   init_xf_stride: int = 16, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_stride: int = 22,
                   xf_stride: int = 16, scale: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None,
                   engine: Optional["HipEngine"] = None):
    """ut_fit_pose_scale, fit_pose with the hand's scale as a parameter: (joint_angles, wrist_xf, scale [n], info [n,6]:
    weighted rms residual, worst residual, iterations, status bits UT_FITS_*, scale information, 0).  init_scale [n] or None
    (= 1); scale_mode UT_SCALE_FREE fits the scale, UT_SCALE_FIXED keeps init_scale.  Every other argument as for fit_pose,
    strided views included; `scale` and `info` may be the caller's buffers."""
    d = _hip_device(targets, "fit_pose_scale")
    if n is None:
        targets = _need(targets, torch.float32, d, "targets").reshape(-1, 63)
    hand_model, init_angles, init_wrist_xf, n, out, limits, mirror, h = _fit_args(
        d, hand_model, init_angles, init_wrist_xf, n, targets.shape[0], [targets], out, limits, mirror, engine)
    if weights is not None:
        weights = _need(weights, torch.float32, d, "weights")
        if tuple(weights.shape) != (n, 21):
            raise ValueError(f"weights must be [{n},21], got {tuple(weights.shape)}")
    if init_scale is not None:
        init_scale = _need(init_scale, torch.float32, d, "init_scale").reshape(-1)
        if init_scale.shape[0] != n:
            raise ValueError("init_scale batch mismatch")
    scale = _out(scale, (n,), torch.float32, d, "scale")
    info = _out(info, (n, 6), torch.float32, d, "info")
    _fit_call("ut_fit_pose_scale", d, h, _ptr(hand_model), hand_model.shape[0], _ptr(targets), target_stride, _ptr(weights),
              _ptr(limits), _ptr(init_scale), int(scale_mode), _ptr(init_angles), init_ja_stride, _ptr(init_wrist_xf),
              init_xf_stride, _ptr(mirror), ctypes.c_float(t_scale), int(max_iters), n, _ptr(out[0]), ja_stride, _ptr(out[1]),
              xf_stride, _ptr(scale), _ptr(info))
    return out[0], out[1], scale, info


def pool_scale(scale: torch.Tensor, info: torch.Tensor, group_size: int, *, group: Optional[torch.Tensor] = None,
               pose_scale: Optional[torch.Tensor] = None, broadcast: bool = True):
    """ut_pool_scale on the outputs of a free fit_pose_scale: scale [G * group_size], info [G * group_size, 6] ->
    (group [G,4]: pooled scale, sigma of ln scale per unit of target noise, scatter, poses used; pose_scale [G * group_size]:
    the group's scale for each of its poses, or None with broadcast=False)."""
    lib = load_library()
    d = _hip_device(scale, "pool_scale")
    scale = _need(scale, torch.float32, d, "scale").reshape(-1)
    info = _need(info, torch.float32, d, "info").reshape(-1, 6)
    if group_size < 1 or scale.shape[0] % group_size or info.shape[0] != scale.shape[0]:
        raise ValueError(f"{scale.shape[0]} scales and {info.shape[0]} info rows do not make groups of {group_size}")
    n_groups = scale.shape[0] // group_size
    group = _out(group, (n_groups, 4), torch.float32, d, "group")
    if broadcast or pose_scale is not None:
        pose_scale = _out(pose_scale, (scale.shape[0],), torch.float32, d, "pose_scale")
    with torch.cuda.device(d):
        rc = lib.ut_pool_scale(None, _ptr(scale), _ptr(info), n_groups, int(group_size), _ptr(group), _ptr(pose_scale), _stream(d))
    _check_rc(lib, None, rc, "ut_pool_scale", "points")
    return group, pose_scale


class Mesh:
    """A hand mesh packed for ut_skin_mesh and resident on one HIP device (ut_mesh_create): sparse bone weights (at most
    MESH_MAX_INFLUENCES per vertex) and the vertex -> triangle table of the normals.  vertices [V,3], triangles [T,3],
    dense_bone_weights [V,17]: numpy arrays or tensors, read on the host.  Raises ValueError when the library refuses the
    mesh (the message says which rule was broken); nothing is launched then.  Freed on close() / garbage collection."""

    def __init__(self, vertices, triangles, dense_bone_weights, device="cuda"):
        self._h = None
        self.lib = load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NativeLibraryError("a Mesh lives on a HIP device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

        def host(x, dtype, tail):
            if isinstance(x, torch.Tensor):
                x = x.detach().cpu().numpy()
            x = np.ascontiguousarray(x, dtype)
            if x.ndim != 2 or x.shape[1] != tail:
                raise ValueError(f"expected an unbatched [*, {tail}] array, got {x.shape}")
            return x
        v, t, w = host(vertices, np.float32, 3), host(triangles, np.int32, 3), host(dense_bone_weights, np.float32, 17)
        if w.shape[0] != v.shape[0]:
            raise ValueError(f"{v.shape[0]} vertices but {w.shape[0]} rows of bone weights")
        h = ctypes.c_void_p()
        rc = self.lib.ut_mesh_create(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], w.ctypes.data, self.device.index,
                                     ctypes.byref(h))
        _check_rc(self.lib, None, rc, "ut_mesh_create", "mesh")
        self._h = h
        self.n_vertices, self.n_triangles = v.shape[0], t.shape[0]

    def counts(self) -> Tuple[int, int]:
        nv, nt = ctypes.c_int(), ctypes.c_int()
        _check_rc(self.lib, None, self.lib.ut_mesh_counts(self._h, ctypes.byref(nv), ctypes.byref(nt)), "ut_mesh_counts")
        return nv.value, nt.value

    def close(self):
        if self._h is not None:
            self.lib.ut_mesh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def skin_mesh(mesh: Mesh, hand_model: torch.Tensor, joint_angles: torch.Tensor, wrist_xf: torch.Tensor,
              mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0, normals: bool = False, ja_stride: int = 22,
              xf_stride: int = 16, n: Optional[int] = None, out: Optional[torch.Tensor] = None,
              out_normals: Optional[torch.Tensor] = None, engine: Optional["HipEngine"] = None):
    """ut_skin_mesh: vertices [n,V,3], or (vertices, normals) with normals=True.  hand_model [1|n,321] (ut_fk's blob);
    joint_angles / wrist_xf either packed [n,22] / [n,4,4], or - with n given - views into a pose-record buffer with explicit
    strides in floats, as for HipEngine.fk.  out / out_normals: preallocated fp32 [n,V,3] to write into.  All tensors on the
    mesh's device; `engine` only lends its handle for error reporting (the kernel needs no network weights)."""
    lib, d = mesh.lib, mesh.device
    if mesh._h is None:
        raise ValueError("the Mesh has been closed")
    hand_model, joint_angles, wrist_xf, mirror, n = _fk_args(d, hand_model, joint_angles, wrist_xf, mirror, n)
    shape = (n, mesh.n_vertices, 3)
    out = _out(out, shape, torch.float32, d, "out")
    if normals or out_normals is not None:
        out_normals = _out(out_normals, shape, torch.float32, d, "out_normals")
    h = engine._h if engine is not None else None
    with torch.cuda.device(d):
        rc = lib.ut_skin_mesh(h, mesh._h, _ptr(hand_model), hand_model.shape[0], _ptr(joint_angles), ja_stride, _ptr(wrist_xf),
                              xf_stride, _ptr(mirror), ctypes.c_float(t_scale), n, _ptr(out), _ptr(out_normals), _stream(d))
    _check_rc(lib, h, rc, "ut_skin_mesh")
    return (out, out_normals) if out_normals is not None else out


UT_CAMERA_FISHEYE62, UT_CAMERA_PINHOLE = 0, 1
RENDER_MAX_VERTICES = 2368


def project_points(points: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor, width: int, height: int,
                   n_points: Optional[int] = None, point_stride: Optional[int] = None, n: Optional[int] = None,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                   engine: Optional["HipEngine"] = None):
    """ut_project_points: world points through cameras -> (window f64 [n,V,P,2] px, eye_z f64 [n,V,P], flags u8 [n,V,P]: bit 0
    in front, bit 1 inside [0,width) x [0,height)).  points fp32 [n,P,3] - or, with n / n_points / point_stride given, any fp32
    view whose row i starts point_stride floats after row i - 1 (keypoints inside pose records are read in place);
    cam_rows i32 [n,V], -1 = unused view; table f64 [R,32] Fisheye62 source cameras or [R,24] pinhole crop cameras (told
    apart by the row length).  A cam_rows entry outside [-1, R) raises IndexError - at once, or from engine.poll_status()
    when `engine` runs deferred checks (then nothing synchronises)."""
    lib, d = load_library(), points.device
    table = _need(table, torch.float64, d, "table")
    if table.dim() != 2 or table.shape[1] not in (24, 32):
        raise ValueError(f"table must be [R,32] source cameras or [R,24] crop cameras, got {tuple(table.shape)}")
    kind = UT_CAMERA_FISHEYE62 if table.shape[1] == 32 else UT_CAMERA_PINHOLE
    if n is None:
        points = _need(points, torch.float32, d, "points")
        if points.dim() != 3 or points.shape[2] != 3:
            raise ValueError(f"points must be [n,P,3], got {tuple(points.shape)}")
        n, n_points = points.shape[0], points.shape[1]
        point_stride = 3 * n_points
    elif points.dtype != torch.float32 or n_points is None or point_stride is None:
        raise ValueError("strided points must be fp32 with n_points and point_stride given")
    cam_rows = _need(cam_rows, torch.int32, d, "cam_rows")
    if cam_rows.dim() != 2 or cam_rows.shape[0] != n:
        raise ValueError(f"cam_rows must be [{n},V], got {tuple(cam_rows.shape)}")
    v = cam_rows.shape[1]
    window, eye_z, flags = out if out is not None else (None, None, None)
    window = _out(window, (n, v, n_points, 2), torch.float64, d, "out[0]")
    eye_z = _out(eye_z, (n, v, n_points), torch.float64, d, "out[1]")
    flags = _out(flags, (n, v, n_points), torch.uint8, d, "out[2]")
    h = engine._h if engine is not None else None
    with torch.cuda.device(d):
        rc = lib.ut_project_points(h, _ptr(points), point_stride, n_points, _ptr(cam_rows), v, _ptr(table), table.shape[0], kind,
                                   n, int(width), int(height), _ptr(window), _ptr(eye_z), _ptr(flags), _stream(d))
    _check_rc(lib, h, rc, "ut_project_points", "points")
    return window, eye_z, flags


TRI_CONVERGED, TRI_AT_MAX_ITERS, TRI_REFUSED, TRI_DEGENERATE = 1, 2, 4, 8      # UT_TRI_*
TRI_MAX_VIEWS = 8


def triangulate_points(window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                       weights: Optional[torch.Tensor] = None, max_iters: int = 16,
                       out: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                       engine: Optional["HipEngine"] = None, *, out_f32: Optional[torch.Tensor] = None,
                       point_stride: Optional[int] = None):
    """ut_triangulate_points, the inverse of project_points: window f64 [n,V,P,2] px (what project_points returns) ->
    (points f64 [n,P,3], info f32 [n,P,4]: weighted rms reprojection residual px, sigma - model units per px of detection noise,
    views used, status bits TRI_*, residual f32 [n,V,P] px per used view).  cam_rows i32 [n,V], -1 = unused view; table f64
    [R,32] Fisheye62 source cameras or [R,24] pinhole crop cameras (told apart by the row length); weights f32 [n,V,P] >= 0 or
    None = all 1 (a window of weight 0 is not read: it may be NaN); V <= TRI_MAX_VIEWS.  out: preallocated (points, info,
    residual), any of them None.  out_f32 with point_stride: an fp32 view whose row i starts point_stride floats after row
    i - 1 and begins with the pose's 3 P floats - keypoints inside records, written in place, or the targets of fit_pose; the
    f64 result rounded once.  A cam_rows entry outside [-1, R) raises IndexError and writes nothing for its pose - at once,
    or from engine.poll_status() when `engine` runs deferred checks (then nothing synchronises)."""
    return _triangulate_points(window, cam_rows, table, weights, max_iters, out, engine, out_f32, point_stride, False)[:3]


def triangulate_points_info(window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                            weights: Optional[torch.Tensor] = None, max_iters: int = 16,
                            out: Optional[Tuple[Optional[torch.Tensor], ...]] = None, engine: Optional["HipEngine"] = None, *,
                            out_f32: Optional[torch.Tensor] = None, point_stride: Optional[int] = None):
    """ut_triangulate_points_info: triangulate_points, bit for bit, that also returns what the views know about each point -
    (points, info, residual, sqrt_info f32 [n,P,6]): (l00, l10, l11, l20, l21, l22) of the lower Cholesky factor L of H = sum_v
    w_v J_v^T J_v at the point, px per model unit; moving the point by d costs |L^T d|^2 px^2 to first order.  All 0 for refused
    and degenerate points and where sigma is +inf.  The input of fit_pose_info.  out: preallocated (points, info, residual,
    sqrt_info), any of them None."""
    return _triangulate_points(window, cam_rows, table, weights, max_iters, out, engine, out_f32, point_stride, True)


def _triangulate_points(window, cam_rows, table, weights, max_iters, out, engine, out_f32, point_stride, factor: bool):
    """triangulate_points and, with factor=True, triangulate_points_info."""
    if window.dim() != 4 or window.shape[3] != 2 or window.dtype != torch.float64:
        raise ValueError(f"window must be f64 [n,V,P,2], got {window.dtype} {tuple(window.shape)}")
    n, v, n_points = window.shape[:3]
    if not 1 <= v <= TRI_MAX_VIEWS or n_points < 1:
        raise ValueError(f"window [n,V,P,2] needs 1 <= V <= {TRI_MAX_VIEWS} and P >= 1, got V = {v}, P = {n_points}")
    if not 1 <= int(max_iters) <= 64:
        raise ValueError(f"max_iters must be in 1..64, got {max_iters}")
    if table.dim() != 2 or table.shape[1] not in (24, 32) or table.shape[0] < 1 or table.dtype != torch.float64:
        raise ValueError(f"table must be f64 [R,32] source cameras or [R,24] crop cameras, got {table.dtype} {tuple(table.shape)}")
    if cam_rows.dtype != torch.int32 or tuple(cam_rows.shape) != (n, v):
        raise ValueError(f"cam_rows must be i32 [{n},{v}], got {cam_rows.dtype} {tuple(cam_rows.shape)}")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (n, v, n_points)):
        raise ValueError(f"weights must be f32 [{n},{v},{n_points}], got {weights.dtype} {tuple(weights.shape)}")
    if (out_f32 is None) != (point_stride is None):
        raise ValueError("out_f32 and point_stride go together")
    if out_f32 is not None and (out_f32.dtype != torch.float32 or point_stride < 3 * n_points
                                or (n and out_f32.numel() and out_f32.stride(-1) != 1)):
        raise ValueError(f"out_f32 must be an fp32 view with point_stride >= {3 * n_points}")
    kind = UT_CAMERA_FISHEYE62 if table.shape[1] == 32 else UT_CAMERA_PINHOLE
    lib = load_library()
    d = _hip_device(window, "triangulate_points_info" if factor else "triangulate_points")
    window, table, cam_rows = _need(window, torch.float64, d, "window"), _need(table, torch.float64, d, "table"), _need(cam_rows, torch.int32, d, "cam_rows")
    if weights is not None:
        weights = _need(weights, torch.float32, d, "weights")
    if out_f32 is not None and out_f32.device != d:
        raise ValueError(f"out_f32 must live on {d}")
    points, info, residual, sqrt_info = tuple(out) + (None,) * (4 - len(out)) if out is not None else (None,) * 4
    points = _out(points, (n, n_points, 3), torch.float64, d, "out[0]")
    info = _out(info, (n, n_points, 4), torch.float32, d, "out[1]")
    residual = _out(residual, (n, v, n_points), torch.float32, d, "out[2]")
    sqrt_info = _out(sqrt_info, (n, n_points, 6), torch.float32, d, "out[3]") if factor else None
    h = engine._h if engine is not None else None
    args = (h, _ptr(window), _ptr(weights), _ptr(cam_rows), v, _ptr(table), table.shape[0], kind, n_points, n, int(max_iters),
            _ptr(points), _ptr(out_f32), int(point_stride or 0), _ptr(info), _ptr(residual))
    with torch.cuda.device(d):
        if not factor:
            rc = lib.ut_triangulate_points(*args, _stream(d))
        else:
            rc = lib.ut_triangulate_points_info(*args, _ptr(sqrt_info), _stream(d))
    _check_rc(lib, h, rc, "ut_triangulate_points_info" if factor else "ut_triangulate_points", "points")
    return points, info, residual, sqrt_info


UT_LOSS_SQUARED, UT_LOSS_HUBER, UT_LOSS_GEMAN_MCCLURE = 0, 1, 2
LOSSES = {"squared": UT_LOSS_SQUARED, "huber": UT_LOSS_HUBER, "geman_mcclure": UT_LOSS_GEMAN_MCCLURE}


def loss_code(loss) -> int:
    """A loss by its name in LOSSES or by its UT_LOSS_* code."""
    if isinstance(loss, str):
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {sorted(LOSSES)}, got {loss!r}")
        return LOSSES[loss]
    if loss not in LOSSES.values():
        raise ValueError(f"loss must be one of {sorted(LOSSES)} or a UT_LOSS_* code, got {loss!r}")
    return int(loss)


def _loss_args(loss, loss_scale) -> Tuple[int, float]:
    """(UT_LOSS_* code, loss_scale) of a loss and its scale, which must be finite and > 0 with a robust loss."""
    code = loss_code(loss)
    if code != UT_LOSS_SQUARED and not (np.isfinite(loss_scale) and loss_scale > 0):
        raise ValueError(f"loss_scale must be finite and > 0, got {loss_scale}")
    return code, float(loss_scale)


def _optional_out(want, shape, d, name: str) -> Optional[torch.Tensor]:
    """An optional f32 output: True = a fresh tensor, a tensor = the caller's own (checked by _out), anything else = None."""
    wanted = want is True or isinstance(want, torch.Tensor)
    return _out(None if want is True else want, shape, torch.float32, d, name) if wanted else None


def _views_inputs(who: str, window, cam_rows, table, weights, loss=None):
    """The detections of the entries in the views, checked: window, table, cam_rows, weights; then `loss` = (loss, loss_scale) where
    the entry checks it here; then the windows' HIP device, `who` naming the entry, and the four tensors on it.  Returns (device,
    window, cam_rows, table, weights, n, V, UT_CAMERA_* kind, _loss_args' pair or None)."""
    if window.dim() != 4 or tuple(window.shape[2:]) != (21, 2) or window.dtype != torch.float64:
        raise ValueError(f"window must be f64 [n,V,21,2], got {window.dtype} {tuple(window.shape)}")
    nw, v = window.shape[:2]
    if not 1 <= v <= TRI_MAX_VIEWS:
        raise ValueError(f"window [n,V,21,2] needs 1 <= V <= {TRI_MAX_VIEWS}, got V = {v}")
    if table.dim() != 2 or table.shape[1] not in (24, 32) or table.shape[0] < 1 or table.dtype != torch.float64:
        raise ValueError(f"table must be f64 [R,32] source cameras or [R,24] crop cameras, got {table.dtype} {tuple(table.shape)}")
    if cam_rows.dtype != torch.int32 or tuple(cam_rows.shape) != (nw, v):
        raise ValueError(f"cam_rows must be i32 [{nw},{v}], got {cam_rows.dtype} {tuple(cam_rows.shape)}")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (nw, v, 21)):
        raise ValueError(f"weights must be f32 [{nw},{v},21], got {weights.dtype} {tuple(weights.shape)}")
    if loss is not None:
        loss = _loss_args(*loss)
    kind = UT_CAMERA_FISHEYE62 if table.shape[1] == 32 else UT_CAMERA_PINHOLE
    d = _hip_device(window, who)
    window, table, cam_rows = _need(window, torch.float64, d, "window"), _need(table, torch.float64, d, "table"), _need(cam_rows, torch.int32, d, "cam_rows")
    weights = None if weights is None else _need(weights, torch.float32, d, "weights")
    return d, window, cam_rows, table, weights, nw, v, kind, loss


def _fit_pose_views(entry, hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights, limits, mirror, t_scale, max_iters,
                    loss=None, scale=None, *, n=None, init_ja_stride=22, init_xf_stride=16, out=None, ja_stride=22, xf_stride=16,
                    info=None, residual=False, engine=None):
    """The three fits in the views into the C `entry`: loss = (code, loss_scale, inlier) for the robust and the scale entry, scale =
    (init_scale, scale_mode, scale) for the scale entry (info [n,6]).  Returns (ja, xf[, scale], info[, residual][, inlier])."""
    if init_angles is None or init_wrist_xf is None:
        raise ValueError("init_angles and init_wrist_xf are required: ut_fit_pose_views has no cold start")
    d, window, cam_rows, table, weights, nw, v, kind, _ = _views_inputs("fit_pose_views", window, cam_rows, table, weights)
    hand_model, init_angles, init_wrist_xf, n, out, limits, mirror, h = _fit_args(
        d, hand_model, init_angles, init_wrist_xf, n, nw, [], out, limits, mirror, engine, windows=True)
    info = _out(info, (n, 4 if scale is None else 6), torch.float32, d, "info")
    residual = _optional_out(residual, (n, v, 21), d, "residual")
    scale_in = loss_in = scale_out = inlier_out = ()
    if loss is not None:
        loss_in, inlier_out = (int(loss[0]), ctypes.c_float(loss[1])), (_optional_out(loss[2], (n, v, 21), d, "inlier"),)
    if scale is not None:
        init_scale, scale_mode, scale = scale
        if init_scale is not None:
            init_scale = _need(init_scale, torch.float32, d, "init_scale").reshape(-1)
            if init_scale.shape[0] != n:
                raise ValueError("init_scale batch mismatch")
        scale_in, scale_out = (_ptr(init_scale), int(scale_mode)), (_out(scale, (n,), torch.float32, d, "scale"),)
    model = (_ptr(hand_model), hand_model.shape[0])      # the C arguments in the header's order, each entry with the pieces it has
    observations = (_ptr(window), _ptr(weights), _ptr(cam_rows), v, _ptr(table), table.shape[0], kind)
    start = (_ptr(init_angles), init_ja_stride, _ptr(init_wrist_xf), init_xf_stride)
    solver = (_ptr(mirror), ctypes.c_float(t_scale), int(max_iters))
    pose_out = (n, _ptr(out[0]), ja_stride, _ptr(out[1]), xf_stride)
    _fit_call(entry, d, h, *model, *observations, _ptr(limits), *scale_in, *start, *solver, *loss_in, *pose_out,
              *map(_ptr, scale_out), _ptr(info), _ptr(residual), *map(_ptr, inlier_out))
    return (out[0], out[1]) + scale_out + (info,) + tuple(t for t in (residual,) + inlier_out if t is not None)


def fit_pose_views(hand_model: torch.Tensor, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                   init_angles: torch.Tensor, init_wrist_xf: torch.Tensor, weights: Optional[torch.Tensor] = None,
                   limits: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                   max_iters: int = 32, *, n: Optional[int] = None, init_ja_stride: int = 22, init_xf_stride: int = 16,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_stride: int = 22, xf_stride: int = 16,
                   info: Optional[torch.Tensor] = None, residual=False, engine: Optional["HipEngine"] = None):
    """ut_fit_pose_views: the pose whose landmarks, projected into the views, meet the detections - fit_pose on the
    reprojection cost sum_v sum_l w_vl |project_v(landmark_l) - window_vl|^2 instead of 3-D targets.  window f64 [n,V,21,2] px,
    cam_rows i32 [n,V] (-1 = unused view), table f64 [R,32] Fisheye62 source cameras or [R,24] pinhole crop cameras (told apart
    by the row length), weights f32 [n,V,21] >= 0 or None = all 1 (a window of weight 0 is not read: it may be NaN); V <=
    TRI_MAX_VIEWS.  init_angles [n,22] / init_wrist_xf [n,4,4] are required: the previous frame's pose, or fit_pose on the
    triangulated landmarks.  hand_model, limits, mirror, t_scale, the strided form (n, init_*_stride, out, *_stride) and the
    pose outputs as for fit_pose.  Returns (joint_angles, wrist_xf, info [n,4]: rms reprojection residual px, largest
    reprojection distance px, iterations, status bits UT_FIT_*) and, with residual=True or a preallocated f32 [n,V,21], the
    reprojection distance of every used observation as a fourth item.  A cam_rows entry outside [-1, R) raises IndexError and
    writes nothing for its pose - at once, or from engine.poll_status() when `engine` runs deferred checks."""
    return _fit_pose_views("ut_fit_pose_views", hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights, limits, mirror,
                           t_scale, max_iters, n=n, init_ja_stride=init_ja_stride, init_xf_stride=init_xf_stride, out=out,
                           ja_stride=ja_stride, xf_stride=xf_stride, info=info, residual=residual, engine=engine)


def fit_pose_views_robust(hand_model: torch.Tensor, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                          init_angles: torch.Tensor, init_wrist_xf: torch.Tensor, weights: Optional[torch.Tensor] = None,
                          limits: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                          max_iters: int = 32, loss="geman_mcclure", loss_scale: float = 3.0, *, inlier=False, **kw):
    """ut_fit_pose_views_robust: fit_pose_views on the cost sum_v sum_l w_vl c^2 rho(d_vl^2 / c^2), d the reprojection distance and
    c = loss_scale in px - a fit that survives a few grossly wrong detections in one launch.  loss: "squared" (fit_pose_views, bit
    for bit), "huber" or "geman_mcclure", or a UT_LOSS_* code; loss_scale must be finite and > 0 with a robust loss.  Everything
    else, **kw included (n, the strides, out, info, residual, engine), as for fit_pose_views, whose tuple comes back - info[0] is
    sqrt(robust cost / sum of the used weights), info[1] and residual stay raw distances - and, with inlier=True or a preallocated
    f32 [n,V,21], psi of every used observation at the returned pose as its last item: 1 for an inlier, towards 0 for an
    outlier, 0 where unused or refused."""
    return _fit_pose_views("ut_fit_pose_views_robust", hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights, limits,
                           mirror, t_scale, max_iters, _loss_args(loss, loss_scale) + (inlier,), **kw)


def fit_pose_views_any_loss(hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights=None, limits=None, mirror=None,
                            t_scale: float = 1.0, max_iters: int = 32, loss="squared", loss_scale: float = 3.0, *, inlier=False, **kw):
    """The fit in the views by the entry that serves `loss`: fit_pose_views for squared without inliers, else fit_pose_views_robust."""
    if loss_code(loss) == UT_LOSS_SQUARED and not inlier:
        return fit_pose_views(hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights, limits, mirror, t_scale, max_iters, **kw)
    return fit_pose_views_robust(hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights, limits, mirror, t_scale,
                                 max_iters, loss, loss_scale, inlier=inlier, **kw)


def fit_pose_views_scale(hand_model: torch.Tensor, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                         init_angles: torch.Tensor, init_wrist_xf: torch.Tensor, weights: Optional[torch.Tensor] = None,
                         limits: Optional[torch.Tensor] = None, init_scale: Optional[torch.Tensor] = None,
                         scale_mode: int = UT_SCALE_FREE, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                         max_iters: int = 32, loss="squared", loss_scale: float = 3.0, *, inlier=False,
                         scale: Optional[torch.Tensor] = None, **kw):
    """ut_fit_pose_views_scale, fit_pose_views_robust with the hand's scale as a parameter: (joint_angles, wrist_xf, scale [n],
    info [n,6]: rms px of the (robust) cost, largest raw reprojection distance px, iterations, status bits UT_FITS_*, scale
    information, 0 - the rows pool_scale reads) and then, as for fit_pose_views_robust, the residual (residual=True or a buffer) and
    the inliers (inlier=True or a buffer).  init_scale [n] or None (= 1); scale_mode UT_SCALE_FREE fits the scale, UT_SCALE_FIXED
    keeps init_scale.  One camera cannot see the hand's size: a free fit on one view returns a scale that means nothing with an
    information near 0 - fix the scale there.  Every other argument, **kw included (n, the strides, out, info, residual, engine),
    as for fit_pose_views_robust; `scale` and `info` may be the caller's buffers."""
    robust = _loss_args(loss, loss_scale) + (inlier,)
    if scale_mode not in (UT_SCALE_FREE, UT_SCALE_FIXED):
        raise ValueError(f"scale_mode must be UT_SCALE_FREE or UT_SCALE_FIXED, got {scale_mode!r}")
    return _fit_pose_views("ut_fit_pose_views_scale", hand_model, window, cam_rows, table, init_angles, init_wrist_xf, weights, limits,
                           mirror, t_scale, max_iters, robust, (init_scale, int(scale_mode), scale), **kw)


UT_COV_OK, UT_COV_SINGULAR, UT_COV_REFUSED = 1, 2, 4
UT_COV_MIN_PIVOT = 2.0 ** -16


def pose_information_views(hand_model: torch.Tensor, joint_angles: torch.Tensor, wrist_xf: torch.Tensor, window: torch.Tensor,
                           cam_rows: torch.Tensor, table: torch.Tensor, weights: Optional[torch.Tensor] = None,
                           angle_sigma: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                           loss="squared", loss_scale: float = 3.0, *, n: Optional[int] = None, ja_stride: int = 22,
                           xf_stride: int = 16, pose_info=True, pivot=True, param_sigma=True, landmark_cov=True, info=True,
                           engine: Optional["HipEngine"] = None):
    """ut_pose_information_views: how well the pose (joint_angles [n,22], wrist_xf [n,4,4]) is known under the cost of
    fit_pose_views_robust on these detections - window, cam_rows, table, weights (informations, px^-2), mirror, t_scale, loss and
    loss_scale exactly as there.  Nothing is fitted.  Returns (pose_info f32 [n,351]: the lower triangle, row-major, of H = sum w
    psi J^T J + the prior on the solver's 26 parameters; pivot [n,3] the rotation increment turns about; param_sigma [n,26] =
    sqrt(diag H^-1); landmark_cov [n,21,6]: (xx, yx, yy, zx, zy, zz) of G_l H^-1 G_l^T; info [n,4]: rms of the cost at the pose,
    the largest landmark sigma, the smallest pivot of the unit-diagonal factor, status UT_COV_OK | UT_COV_SINGULAR (sigmas and
    covariances +inf) | UT_COV_REFUSED (everything 0)).  Each output: True = a fresh tensor, False = left out (None comes back;
    not all five), or a preallocated contiguous f32 tensor.  angle_sigma f32 [1|n,20] (one row per model row) or None: the
    sigma in rad of a Gaussian prior on each joint angle.  With n given, joint_angles / wrist_xf are fp32 views read in place with
    the strides given in floats - pose records, or a fit's strided outputs.  A cam_rows entry outside [-1, R) raises IndexError
    and writes nothing for its pose - at once, or from engine.poll_status() when `engine` runs deferred checks."""
    if joint_angles is None or wrist_xf is None:
        raise ValueError("joint_angles and wrist_xf are required")
    d, window, cam_rows, table, weights, nw, v, kind, (code, loss_scale) = _views_inputs(
        "pose_information_views", window, cam_rows, table, weights, (loss, loss_scale))
    hand_model, joint_angles, wrist_xf, mirror, n = _fk_args(d, hand_model, joint_angles, wrist_xf, mirror, n)
    if n != nw:
        raise ValueError(f"{n} poses for {nw} poses' windows")
    if angle_sigma is not None:
        angle_sigma = _need(angle_sigma, torch.float32, d, "angle_sigma").reshape(-1, 20)
        if angle_sigma.shape[0] != hand_model.shape[0]:
            raise ValueError(f"angle_sigma has {angle_sigma.shape[0]} rows for {hand_model.shape[0]} model rows")
    outs = tuple(_optional_out(want, shape, d, name) for name, want, shape in (("pose_info", pose_info, (n, 351)), ("pivot", pivot, (n, 3)), (
        "param_sigma", param_sigma, (n, 26)), ("landmark_cov", landmark_cov, (n, 21, 6)), ("info", info, (n, 4))))
    if all(o is None for o in outs):
        raise ValueError("at least one output is needed")
    h = engine._h if engine is not None else None
    _fit_call("ut_pose_information_views", d, h, _ptr(hand_model), hand_model.shape[0], _ptr(window), _ptr(weights), _ptr(cam_rows), v,
              _ptr(table), table.shape[0], kind, _ptr(angle_sigma), _ptr(joint_angles), ja_stride, _ptr(wrist_xf), xf_stride,
              _ptr(mirror), ctypes.c_float(t_scale), code, ctypes.c_float(loss_scale), n, *map(_ptr, outs))
    return outs


UT_SMOOTH_OK, UT_SMOOTH_SINGULAR, UT_SMOOTH_REFUSED, UT_SMOOTH_GAP = 1, 2, 4, 8
UT_SMOOTH_WORK = 408


def smooth_pose_sequence(joint_angles: torch.Tensor, wrist_xf: torch.Tensor, pose_info: torch.Tensor, pivot: torch.Tensor,
                         step_var: torch.Tensor, frame_weight: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
                         centre: Optional[torch.Tensor] = None, t_scale: float = 1.0, *, n_seq: Optional[int] = None,
                         n_frames: Optional[int] = None, ja_stride: int = 22, xf_stride: int = 16,
                         out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_out_stride: int = 22, xf_out_stride: int = 16,
                         param_sigma=False, info=True, workspace: Optional[torch.Tensor] = None, engine: Optional["HipEngine"] = None):
    """ut_smooth_pose_sequence: the fitted poses of n_seq sequences of n_frames frames (joint_angles [n_seq,T,22], wrist_xf
    [n_seq,T,4,4]) combined by their information matrices (pose_info [n_seq,T,351] and pivot [n_seq,T,3] of
    pose_information_views) under a random walk with the variances step_var f32 [1|n_seq,26] per frame step (rad^2, rad^2, target
    units^2) - include/umetrack_hip_smooth.h states the model.  frame_weight f32 [n_seq,T] >= 0 or None = 1 (0: the frame is a
    gap), lengths i32 [n_seq] or None, centre f32 [n_seq,3] or None: the body-fixed point the motion model speaks about, in the
    proper wrist frame and target units.  Returns (joint_angles, wrist_xf, param_sigma [n_seq,T,26] or None, info [n_seq,T,4] or
    None: sqrt(u^T H' u), sqrt(m^T W m) of the smoothed step, the smallest scaled pivot, status bits UT_SMOOTH_*).  param_sigma /
    info: True = a fresh tensor, False = left out, or a preallocated contiguous f32 tensor.  out: preallocated (joint_angles,
    wrist_xf) - they may be the inputs themselves.  With n_seq and n_frames given, the poses are fp32 views read in place (and `out`
    written) with the strides given in floats.  workspace: a contiguous f32 tensor of at least n_seq * T * UT_SMOOTH_WORK elements,
    or None = a fresh one.  No device status word: nothing synchronises, the call is capturable."""
    d = _hip_device(pose_info, "smooth_pose_sequence")
    if n_seq is None or n_frames is None:
        if joint_angles.dim() != 3 or joint_angles.shape[2] != 22:
            raise ValueError(f"joint_angles must be [n_seq,T,22], got {tuple(joint_angles.shape)}")
        n_seq, n_frames = joint_angles.shape[:2]
        joint_angles = _need(joint_angles, torch.float32, d, "joint_angles")
        wrist_xf = _need(wrist_xf, torch.float32, d, "wrist_xf")
        if tuple(wrist_xf.shape) != (n_seq, n_frames, 4, 4):
            raise ValueError(f"wrist_xf must be [{n_seq},{n_frames},4,4], got {tuple(wrist_xf.shape)}")
    elif joint_angles.device != d or wrist_xf.device != d or joint_angles.dtype != torch.float32 or wrist_xf.dtype != torch.float32:
        raise ValueError(f"strided pose views must be fp32 on {d}")
    n = n_seq * n_frames
    if n_frames < 1:
        raise ValueError("n_frames must be at least 1")
    pose_info, pivot = _need(pose_info, torch.float32, d, "pose_info"), _need(pivot, torch.float32, d, "pivot")
    if pose_info.numel() != n * 351 or pivot.numel() != n * 3:
        raise ValueError(f"pose_info / pivot must hold [{n_seq},{n_frames},351] / [{n_seq},{n_frames},3]")
    step_var = _need(step_var, torch.float32, d, "step_var").reshape(-1, 26)
    if step_var.shape[0] not in (1, n_seq) and n_seq:
        raise ValueError(f"step_var has {step_var.shape[0]} rows for {n_seq} sequences")
    if frame_weight is not None:
        frame_weight = _need(frame_weight, torch.float32, d, "frame_weight")
        if frame_weight.numel() != n:
            raise ValueError(f"frame_weight must be [{n_seq},{n_frames}]")
    if lengths is not None:
        lengths = _need(lengths, torch.int32, d, "lengths")
        if lengths.numel() != n_seq:
            raise ValueError(f"lengths must be [{n_seq}]")
    if centre is not None:
        centre = _need(centre, torch.float32, d, "centre")
        if centre.numel() != n_seq * 3:
            raise ValueError(f"centre must be [{n_seq},3]")
    if out is None:
        out = (torch.empty((n_seq, n_frames, 22), dtype=torch.float32, device=d), torch.empty((n_seq, n_frames, 4, 4), dtype=torch.float32, device=d))
        ja_out_stride, xf_out_stride = 22, 16
    elif any(o.device != d or o.dtype != torch.float32 for o in out):
        raise ValueError(f"out must be fp32 on {d}")
    if workspace is None:
        workspace = torch.empty((max(n, 1), UT_SMOOTH_WORK), dtype=torch.float32, device=d)
    elif workspace.device != d or workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.numel() < n * UT_SMOOTH_WORK:
        raise ValueError(f"workspace must be a contiguous f32 tensor of at least {n * UT_SMOOTH_WORK} elements on {d}")
    param_sigma = _optional_out(param_sigma, (n_seq, n_frames, 26), d, "param_sigma")
    info = _optional_out(info, (n_seq, n_frames, 4), d, "info")
    h = engine._h if engine is not None else None
    _fit_call("ut_smooth_pose_sequence", d, h, _ptr(joint_angles), ja_stride, _ptr(wrist_xf), xf_stride, _ptr(pose_info), _ptr(pivot),
              _ptr(frame_weight), _ptr(lengths), _ptr(centre), _ptr(step_var), step_var.shape[0], ctypes.c_float(t_scale), n_seq, n_frames,
              _ptr(workspace), _ptr(out[0]), ja_out_stride, _ptr(out[1]), xf_out_stride, _ptr(param_sigma), _ptr(info))
    return out[0], out[1], param_sigma, info


UT_START_MAX_SEEDS = 64


def start_pose_views(hand_model: torch.Tensor, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor,
                     bank_angles: torch.Tensor, seeds: torch.Tensor, weights: Optional[torch.Tensor] = None,
                     limits: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0,
                     iters: int = 30, *, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_stride: int = 22,
                     xf_stride: int = 16, info: Optional[torch.Tensor] = None, engine: Optional["HipEngine"] = None):
    """ut_start_pose_views: starts for fit_pose_views from the detections alone - generalised PnP by orthogonal iteration, one start
    per hand and bank pose, the best of the rotation seeds by the exact reprojection cost.  window, cam_rows, table, weights,
    hand_model, limits, mirror, t_scale as for fit_pose_views; bank_angles f32 [K,20]; seeds f64 [S,3,3] proper rotations, S <=
    UT_START_MAX_SEEDS.  Returns (joint_angles [n*K,22], wrist_xf [n*K,4,4], info [n*K,4]: rms px of the start, largest
    reprojection distance px, the winning seed, status 0 or UT_FIT_REFUSED), row i*K + k the start of hand i from bank pose k -
    what fit_pose_views takes as its init.  out: preallocated fp32 views written with the strides given in floats.  A cam_rows
    entry outside [-1, R) raises IndexError and writes nothing for its hand - at once, or from engine.poll_status() when `engine`
    runs deferred checks (then nothing synchronises and the launch is capturable)."""
    d, window, cam_rows, table, weights, n, v, kind, _ = _views_inputs("start_pose_views", window, cam_rows, table, weights)
    hand_model = _need(hand_model, torch.float32, d, "hand_model").reshape(-1, 321)
    if hand_model.shape[0] not in (1, n) and n:
        raise ValueError(f"hand_model has {hand_model.shape[0]} rows for {n} hands")
    bank_angles = _need(bank_angles, torch.float32, d, "bank_angles")
    if bank_angles.dim() != 2 or bank_angles.shape[1] != 20 or bank_angles.shape[0] < 1:
        raise ValueError(f"bank_angles must be [K,20] with K >= 1, got {tuple(bank_angles.shape)}")
    seeds = _need(seeds, torch.float64, d, "seeds")
    if seeds.numel() % 9 or not 1 <= seeds.numel() // 9 <= UT_START_MAX_SEEDS:
        raise ValueError(f"seeds must be f64 [S,3,3] with 1 <= S <= {UT_START_MAX_SEEDS}, got {tuple(seeds.shape)}")
    if not 1 <= int(iters) <= 256:
        raise ValueError(f"iters must be in 1..256, got {iters}")
    k = bank_angles.shape[0]
    if limits is not None:
        limits = _need(limits, torch.float32, d, "limits").reshape(-1, 20, 2)
        if limits.shape[0] != hand_model.shape[0]:
            raise ValueError(f"limits has {limits.shape[0]} rows for {hand_model.shape[0]} model rows")
    if mirror is not None:
        mirror = _need(mirror, torch.int64, d, "mirror").reshape(-1)
        if mirror.shape[0] != n:
            raise ValueError("mirror batch mismatch")
    if out is None:
        out = (torch.empty(n * k, 22, dtype=torch.float32, device=d), torch.empty(n * k, 4, 4, dtype=torch.float32, device=d))
        ja_stride, xf_stride = 22, 16
    elif any(o.device != d or o.dtype != torch.float32 for o in out):
        raise ValueError(f"out must be fp32 on {d}")
    info = _out(info, (n * k, 4), torch.float32, d, "info")
    _fit_call("ut_start_pose_views", d, engine._h if engine is not None else None, _ptr(hand_model), hand_model.shape[0], _ptr(window),
              _ptr(weights), _ptr(cam_rows), v, _ptr(table), table.shape[0], kind, _ptr(limits), _ptr(bank_angles), k, _ptr(seeds),
              seeds.numel() // 9, _ptr(mirror), ctypes.c_float(t_scale), int(iters), n, _ptr(out[0]), ja_stride, _ptr(out[1]), xf_stride,
              _ptr(info))
    return out[0], out[1], info


def select_pose(joint_angles: torch.Tensor, wrist_xf: torch.Tensor, info: torch.Tensor, n_cand: int, *,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, out_info: Optional[torch.Tensor] = None,
                out_index: Optional[torch.Tensor] = None):
    """ut_select_pose: of n_cand fitted candidates per hand (joint_angles [n*n_cand,22], wrist_xf [n*n_cand,4,4], info
    [n*n_cand,4], rows i*n_cand + c) the one with the lowest info[:,0] among those that are not UT_FIT_REFUSED, the lowest index
    among equals.  Returns (joint_angles [n,22], wrist_xf [n,4,4], info [n,4], index i32 [n]); index -1 and candidate 0 where
    every candidate is refused.  No status word: nothing synchronises, the call is capturable."""
    d = _hip_device(info, "select_pose")
    joint_angles = _need(joint_angles, torch.float32, d, "joint_angles").reshape(-1, 22)
    wrist_xf = _need(wrist_xf, torch.float32, d, "wrist_xf").reshape(-1, 16)
    info = _need(info, torch.float32, d, "info").reshape(-1, 4)
    n_cand = int(n_cand)
    rows = info.shape[0]
    if n_cand < 1 or rows % n_cand or joint_angles.shape[0] != rows or wrist_xf.shape[0] != rows:
        raise ValueError(f"{rows} info rows, {joint_angles.shape[0]} / {wrist_xf.shape[0]} poses and n_cand = {n_cand} do not go together")
    n = rows // n_cand
    ja = _out(None if out is None else out[0], (n, 22), torch.float32, d, "out[0]")
    xf = _out(None if out is None else out[1], (n, 4, 4), torch.float32, d, "out[1]")
    out_info = _out(out_info, (n, 4), torch.float32, d, "out_info")
    out_index = _out(out_index, (n,), torch.int32, d, "out_index")
    lib = load_library()
    with torch.cuda.device(d):
        rc = lib.ut_select_pose(_ptr(joint_angles), 22, _ptr(wrist_xf), 16, _ptr(info), n, n_cand, _ptr(ja), 22, _ptr(xf), 16,
                                _ptr(out_info), _ptr(out_index), _stream(d))
    _check_rc(lib, None, rc, "ut_select_pose", "points")
    return ja, xf, out_info, out_index


UT_TRACK_WARM, UT_TRACK_COLD, UT_TRACK_NONE = 0, 1, 2


def track_pose_views(hand_model: torch.Tensor, window: torch.Tensor, cam_rows: torch.Tensor, table: torch.Tensor, n_frames: int,
                     init_angles: Optional[torch.Tensor] = None, init_wrist_xf: Optional[torch.Tensor] = None, cold=None,
                     weights: Optional[torch.Tensor] = None, limits: Optional[torch.Tensor] = None, mirror: Optional[torch.Tensor] = None,
                     lengths: Optional[torch.Tensor] = None, t_scale: float = 1.0, max_iters: int = 32, loss="squared",
                     loss_scale: float = 3.0, recover_ratio: float = 1.5, recover_floor: float = 0.01, *, init_ja_stride: int = 22,
                     init_xf_stride: int = 16, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ja_stride: int = 22,
                     xf_stride: int = 16, info: Optional[torch.Tensor] = None, chosen: Optional[torch.Tensor] = None,
                     engine: Optional["HipEngine"] = None):
    """ut_track_pose_views: n_seq sequences of n_frames frames of detections followed frame by frame in ONE launch - the warm fit of
    fit_pose_views_robust from the previous frame's choice, the cold row taken where the warm fit is refused or its rms exceeds
    recover_ratio x the cold rms + recover_floor (include/umetrack_hip_track.h states the rule; the result is that chain of
    launches bit for bit).  window f64 [n_seq * n_frames,V,21,2], cam_rows, weights, mirror and hand_model / limits rows: frame t of
    sequence s is row s * n_frames + t, everything else as for fit_pose_views_robust.  init_angles [n_seq,22] / init_wrist_xf
    [n_seq,4,4]: the start of each sequence's frame 0, or None: the first usable cold row starts it.  cold = (joint_angles [n,22],
    wrist_xf [n,4,4], info [n,4], index i32 [n]), what select_pose returns at the end of the cold chain on the same rows, or None:
    no recovery.  lengths i32 [n_seq] or None.  Returns (joint_angles [n,22], wrist_xf [n,4,4], info [n,4], chosen i32 [n]:
    UT_TRACK_WARM / UT_TRACK_COLD / UT_TRACK_NONE, -1 at or past a sequence's length, where nothing else is written but an info row
    of 0).  out: preallocated fp32 views written with the strides given in floats, the init pair read with init_*_stride when they
    are not the packed shapes.  A cam_rows entry outside [-1, R) inside a sequence's length raises IndexError and writes nothing
    for that sequence - at once, or from engine.poll_status() when `engine` runs deferred checks (then nothing synchronises and the
    launch is capturable)."""
    d, window, cam_rows, table, weights, n, v, kind, (code, loss_scale) = _views_inputs(
        "track_pose_views", window, cam_rows, table, weights, (loss, loss_scale))
    n_frames = int(n_frames)
    if n_frames < 1 or n % n_frames:
        raise ValueError(f"{n} rows of windows are not sequences of {n_frames} frames")
    n_seq = n // n_frames
    hand_model = _need(hand_model, torch.float32, d, "hand_model").reshape(-1, 321)
    if hand_model.shape[0] not in (1, n) and n:
        raise ValueError(f"hand_model has {hand_model.shape[0]} rows for {n} frames")
    if (init_angles is None) != (init_wrist_xf is None):
        raise ValueError("init_angles and init_wrist_xf go together")
    if init_angles is None and cold is None:
        raise ValueError("an init or the cold chain's results are needed: there is nothing to start from")
    if init_angles is not None:
        if (init_ja_stride, init_xf_stride) == (22, 16):
            init_angles = _need(init_angles, torch.float32, d, "init_angles").reshape(-1, 22)
            init_wrist_xf = _need(init_wrist_xf, torch.float32, d, "init_wrist_xf").reshape(-1, 16)
            if init_angles.shape[0] != n_seq or init_wrist_xf.shape[0] != n_seq:
                raise ValueError(f"init_angles / init_wrist_xf must hold one row per sequence ({n_seq})")
        elif any(t.device != d or t.dtype != torch.float32 for t in (init_angles, init_wrist_xf)):
            raise ValueError(f"strided init views must be fp32 on {d}")
    if cold is not None:
        cja, cxf, cinfo, cindex = cold
        cja, cxf = _need(cja, torch.float32, d, "cold[0]").reshape(-1, 22), _need(cxf, torch.float32, d, "cold[1]").reshape(-1, 16)
        cinfo, cindex = _need(cinfo, torch.float32, d, "cold[2]").reshape(-1, 4), _need(cindex, torch.int32, d, "cold[3]").reshape(-1)
        if any(t.shape[0] != n for t in (cja, cxf, cinfo, cindex)):
            raise ValueError(f"the cold results must hold one row per frame ({n})")
        cold = (cja, cxf, cinfo, cindex)
    else:
        cold = (None, None, None, None)
    if not (np.isfinite(recover_ratio) and recover_ratio >= 1.0):
        raise ValueError(f"recover_ratio must be finite and at least 1, got {recover_ratio}")
    if not (np.isfinite(recover_floor) and recover_floor >= 0.0):
        raise ValueError(f"recover_floor must be finite and not negative, got {recover_floor}")
    if limits is not None:
        limits = _need(limits, torch.float32, d, "limits").reshape(-1, 20, 2)
        if limits.shape[0] != hand_model.shape[0]:
            raise ValueError(f"limits has {limits.shape[0]} rows for {hand_model.shape[0]} model rows")
    if mirror is not None:
        mirror = _need(mirror, torch.int64, d, "mirror").reshape(-1)
        if mirror.shape[0] != n:
            raise ValueError("mirror batch mismatch")
    if lengths is not None:
        lengths = _need(lengths, torch.int32, d, "lengths").reshape(-1)
        if lengths.shape[0] != n_seq:
            raise ValueError(f"lengths must be [{n_seq}]")
    if out is None:
        out = (torch.empty(n, 22, dtype=torch.float32, device=d), torch.empty(n, 4, 4, dtype=torch.float32, device=d))
        ja_stride, xf_stride = 22, 16
    elif any(o.device != d or o.dtype != torch.float32 for o in out):
        raise ValueError(f"out must be fp32 on {d}")
    info = _out(info, (n, 4), torch.float32, d, "info")
    chosen = _out(chosen, (n,), torch.int32, d, "chosen")
    _fit_call("ut_track_pose_views", d, engine._h if engine is not None else None, _ptr(hand_model), hand_model.shape[0], _ptr(window),
              _ptr(weights), _ptr(cam_rows), v, _ptr(table), table.shape[0], kind, _ptr(limits), _ptr(init_angles), init_ja_stride,
              _ptr(init_wrist_xf), init_xf_stride, _ptr(cold[0]), 22, _ptr(cold[1]), 16, _ptr(cold[2]), _ptr(cold[3]),
              ctypes.c_double(recover_ratio), ctypes.c_double(recover_floor), _ptr(lengths), _ptr(mirror), ctypes.c_float(t_scale),
              int(max_iters), code, ctypes.c_float(loss_scale), n_seq, n_frames, _ptr(out[0]), ja_stride, _ptr(out[1]), xf_stride,
              _ptr(info), _ptr(chosen))
    return out[0], out[1], info, chosen


def render_mesh(mesh: Mesh, vertices: torch.Tensor, crop_params: torch.Tensor, sample_range: torch.Tensor,
                crop_size: int = 96, depth=True, tri=True, shade=True, engine: Optional["HipEngine"] = None):
    """ut_render_mesh: posed meshes [n,V,3] (world, fp32) rasterised into their crop cameras (crop_params f64 [N,24];
    sample_range i64 [n,2], 0 - 2 crops per pose) -> (depth f32, tri i32, shade u8), each [N,96,96] or None.
    depth / tri / shade: True = allocate (crops no pose names keep the background: +inf, -1, 0), False = leave out, or a
    preallocated contiguous tensor to write into (crops no pose names are then left as they are).  A bad sample_range raises
    IndexError and draws nothing - at once, or from engine.poll_status() when `engine` runs deferred checks."""
    lib, d = mesh.lib, mesh.device
    if mesh._h is None:
        raise ValueError("the Mesh has been closed")
    vertices = _need(vertices, torch.float32, d, "vertices")
    if vertices.dim() != 3 or tuple(vertices.shape[1:]) != (mesh.n_vertices, 3):
        raise ValueError(f"vertices must be [n,{mesh.n_vertices},3], got {tuple(vertices.shape)}")
    n = vertices.shape[0]
    crop_params = _need(crop_params, torch.float64, d, "crop_params").reshape(-1, 24)
    sample_range = _need(sample_range, torch.int64, d, "sample_range")
    if tuple(sample_range.shape) != (n, 2):
        raise ValueError(f"sample_range must be [{n},2], got {tuple(sample_range.shape)}")
    n_crops = crop_params.shape[0]
    shape = (n_crops, crop_size, crop_size)

    def buf(t, dtype, fill, name):      # True: allocate with the background value; False / None: leave the output out
        if t is False or t is None:
            return None
        return _out(None if t is True else t, shape, dtype, d, name, fill)
    depth, tri, shade = buf(depth, torch.float32, float("inf"), "depth"), buf(tri, torch.int32, -1, "tri"), buf(shade, torch.uint8, 0, "shade")
    h = engine._h if engine is not None else None
    with torch.cuda.device(d):
        rc = lib.ut_render_mesh(h, mesh._h, _ptr(vertices), _ptr(crop_params), n_crops, _ptr(sample_range), n, crop_size,
                                _ptr(depth), _ptr(tri), _ptr(shade), _stream(d))
    _check_rc(lib, h, rc, "ut_render_mesh", "points")
    return depth, tri, shade


def _crop_outputs(out, n: int, v: int, d, fill=None, landmarks: bool = False) -> Dict[str, torch.Tensor]:
    """The outputs of the two crop-camera entries for n hands x v view slots.  out None: fresh tensors (the camera rows
    filled with `fill` if one is given).  Otherwise the caller's tensors under the same keys, written in place and never
    pre-filled; each is checked for dtype, device, contiguity and its element count for n rows, so leading-row views of
    staging buffers laid out [n,V,9] / [n,V,16] pass."""
    spec = {"crop_params": ((n, v, 24), torch.float64, fill), "intrinsics": ((n, v, 3, 3), torch.float32, fill),
            "extrinsics": ((n, v, 4, 4), torch.float32, fill), "cam_index": ((n, v), torch.int32, None),
            "n_views": ((n,), torch.int32, None), "status": ((n,), torch.int32, None)}
    if landmarks:
        spec["landmarks"] = ((n, arch.N_LANDMARKS, 3), torch.float32, None)
    return {k: _out(None if out is None else out[k], shape, dtype, d, k, fill_k, flat=True)
            for k, (shape, dtype, fill_k) in spec.items()}


def gen_crop_cameras(cam_params: torch.Tensor, camera_angles: torch.Tensor, hand_model: torch.Tensor,
                     joint_limits: torch.Tensor, joint_angles: torch.Tensor, wrist_xf: torch.Tensor,
                     frame_idx: torch.Tensor, hand_idx: torch.Tensor, n_cams: int, src_wh: Tuple[int, int],
                     max_views: int = 2, min_vis: int = 19, crop_size: int = arch.CROP,
                     focal_multiplier: float = 0.8, check_indices: bool = True,
                     want_landmarks: bool = False, *, out: Optional[Dict[str, torch.Tensor]] = None
                     ) -> Dict[str, torch.Tensor]:
    """ut_gen_crop_cameras: crop cameras of n (frame, hand) label poses in one launch, padded to max_views.
    Returns crop_params [n,V,24] f64, intrinsics [n,V,3,3], extrinsics [n,V,4,4], cam_index [n,V] i32,
    n_views [n] i32, status [n] i32 (and landmarks [n,21,3] with want_landmarks).  out: preallocated tensors under these
    keys to write into (see _crop_outputs).  All tensors on one HIP device; no CPU fallback."""
    lib = load_library()
    d = _hip_device(joint_angles, "gen_crop_cameras")
    cam_params = _need(cam_params, torch.float64, d, "cam_params").reshape(-1, 32)
    camera_angles = _need(camera_angles, torch.float64, d, "camera_angles").reshape(-1)
    hand_model = _need(hand_model, torch.float32, d, "hand_model").reshape(-1, 321)
    joint_limits = _need(joint_limits, torch.float32, d, "joint_limits").reshape(-1, 44)
    joint_angles = _need(joint_angles, torch.float32, d, "joint_angles").reshape(-1, 22)
    wrist_xf = _need(wrist_xf, torch.float32, d, "wrist_xf").reshape(-1, 16)
    frame_idx = _need(frame_idx, torch.int32, d, "frame_idx").reshape(-1)
    hand_idx = _need(hand_idx, torch.int64, d, "hand_idx").reshape(-1)
    n = joint_angles.shape[0]
    if not (wrist_xf.shape[0] == frame_idx.shape[0] == hand_idx.shape[0] == n):
        raise ValueError("gen_crop_cameras: joint_angles, wrist_xf, frame_idx and hand_idx disagree on n")
    if hand_model.shape[0] != joint_limits.shape[0] or hand_model.shape[0] not in (1, n):
        raise ValueError("gen_crop_cameras: hand_model / joint_limits must hold 1 or n models")
    if camera_angles.shape[0] != n_cams or cam_params.shape[0] % n_cams:
        raise ValueError("gen_crop_cameras: cam_params rows must be a multiple of n_cams = len(camera_angles)")
    # (reads frame_idx back: pass check_indices=False when the same index tensor was validated before)
    if check_indices and n and (int(frame_idx.max()) + 1) * n_cams > cam_params.shape[0]:
        raise ValueError("gen_crop_cameras: frame_idx points past cam_params")
    out = _crop_outputs(out, n, max_views, d, fill=0, landmarks=want_landmarks)      # unused view slots stay zero
    with torch.cuda.device(d):
        rc = lib.ut_gen_crop_cameras(None, _ptr(cam_params), _ptr(camera_angles), _ptr(hand_model), _ptr(joint_limits),
                                     hand_model.shape[0], _ptr(joint_angles), _ptr(wrist_xf), _ptr(frame_idx),
                                     _ptr(hand_idx), n, n_cams, max_views, min_vis, int(src_wh[0]), int(src_wh[1]),
                                     crop_size, ctypes.c_double(focal_multiplier), _ptr(out["crop_params"]),
                                     _ptr(out["intrinsics"]), _ptr(out["extrinsics"]), _ptr(out["cam_index"]),
                                     _ptr(out["n_views"]), _ptr(out["status"]), _ptr(out.get("landmarks")), _stream(d))
    _check_rc(lib, None, rc, "ut_gen_crop_cameras")
    return out


def gen_crop_cameras_from_window_points(cam_params: torch.Tensor, keypoints: torch.Tensor, src_row: torch.Tensor,
                                        hand_idx: torch.Tensor, crop_size: int = arch.CROP,
                                        focal_multiplier: float = 0.8, check_indices: bool = True, *,
                                        out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """ut_gen_crop_cameras_from_window_points: crop cameras of n hand candidates placed from 21 window keypoints per
    view (lib/tracker/tracker.py:111-219), one launch.  cam_params [R,32] f64, keypoints [n,V,21,2] (window px),
    src_row [n,V] (row of cam_params, -1 = not seen in that view), hand_idx [n].  Returns crop_params [n,V,24] f64,
    intrinsics [n,V,3,3], extrinsics [n,V,4,4], cam_index [n,V] i32 (the src_row of each filled slot, -1 after),
    n_views [n] i32, status [n] i32.  out: preallocated tensors under these keys to write into (see _crop_outputs).  All
    tensors on one HIP device; no CPU fallback."""
    lib = load_library()
    d = _hip_device(keypoints, "gen_crop_cameras_from_window_points")
    if keypoints.dim() != 4 or tuple(keypoints.shape[2:]) != (arch.N_LANDMARKS, 2):
        raise ValueError("keypoints must be [n, views, 21, 2]")
    n, v = keypoints.shape[:2]
    cam_params = _need(cam_params, torch.float64, d, "cam_params").reshape(-1, 32)
    keypoints = _need(keypoints, torch.float64, d, "keypoints")
    src_row = _need(src_row, torch.int32, d, "src_row")
    hand_idx = _need(hand_idx, torch.int64, d, "hand_idx").reshape(-1)
    if tuple(src_row.shape) != (n, v) or hand_idx.shape[0] != n:
        raise ValueError("gen_crop_cameras_from_window_points: keypoints, src_row and hand_idx disagree on n / views")
    # (reads the indices back: pass check_indices=False when the same tensors were validated before; the C entry
    # checks them again before it launches and then fails with UT_E_INVALID instead)
    if check_indices and n:
        if int(src_row.min()) < -1 or int(src_row.max()) >= cam_params.shape[0]:
            raise ValueError("gen_crop_cameras_from_window_points: src_row points past cam_params")
        if bool(((hand_idx != 0) & (hand_idx != 1)).any()):
            raise ValueError("gen_crop_cameras_from_window_points: hand_idx must be 0 or 1")
    out = _crop_outputs(out, n, v, d)
    with torch.cuda.device(d):
        rc = lib.ut_gen_crop_cameras_from_window_points(
            None, _ptr(cam_params), cam_params.shape[0], _ptr(keypoints), _ptr(src_row), _ptr(hand_idx), n, v,
            crop_size, ctypes.c_double(focal_multiplier), _ptr(out["crop_params"]), _ptr(out["intrinsics"]),
            _ptr(out["extrinsics"]), _ptr(out["cam_index"]), _ptr(out["n_views"]), _ptr(out["status"]), _stream(d))
    _check_rc(lib, None, rc, "ut_gen_crop_cameras_from_window_points")
    return out


def gen_crop_matrices(orig_extrinsics: torch.Tensor, orig_intrinsics: torch.Tensor, crop_points: torch.Tensor,
                      hand_idx: torch.Tensor, crop_size: int = arch.CROP, focal_multiplier: float = 0.95
                      ) -> Dict[str, torch.Tensor]:
    """ut_gen_crop_matrices.  orig_extrinsics [F,V,4,4], orig_intrinsics [F,V,3,3], crop_points [F,P,3], hand_idx [F]
    -> extrinsics_xf [F,V,4,4], new_intrinsics [F,V,3,3], resample_xf [F,V,4,4], status [F,V] (i32)."""
    lib = load_library()
    d = _hip_device(orig_extrinsics, "gen_crop_matrices")
    if orig_extrinsics.dim() != 4 or tuple(orig_extrinsics.shape[2:]) != (4, 4):
        raise ValueError("orig_extrinsics must be [frames, views, 4, 4]")
    f, v = orig_extrinsics.shape[:2]
    if tuple(orig_intrinsics.shape) != (f, v, 3, 3):
        raise ValueError("orig_intrinsics must be [frames, views, 3, 3]")
    if crop_points.dim() != 3 or crop_points.shape[0] != f or crop_points.shape[2] != 3 or crop_points.shape[1] < 1:
        raise ValueError("crop_points must be [frames, points, 3]")
    ext = _need(orig_extrinsics, torch.float32, d, "orig_extrinsics")
    intr = _need(orig_intrinsics, torch.float32, d, "orig_intrinsics")
    pts = _need(crop_points, torch.float32, d, "crop_points")
    hand = _need(hand_idx, torch.int64, d, "hand_idx").reshape(-1)
    if hand.shape[0] != f:
        raise ValueError("hand_idx must be [frames]")
    out = {"extrinsics_xf": torch.empty(f, v, 4, 4, device=d), "new_intrinsics": torch.empty(f, v, 3, 3, device=d),
           "resample_xf": torch.empty(f, v, 4, 4, device=d), "status": torch.empty(f, v, dtype=torch.int32, device=d)}
    with torch.cuda.device(d):
        rc = lib.ut_gen_crop_matrices(None, _ptr(ext), _ptr(intr), _ptr(pts), _ptr(hand), f, v, pts.shape[1], crop_size,
                                      ctypes.c_double(focal_multiplier), _ptr(out["extrinsics_xf"]),
                                      _ptr(out["new_intrinsics"]), _ptr(out["resample_xf"]), _ptr(out["status"]), _stream(d))
    _check_rc(lib, None, rc, "ut_gen_crop_matrices")
    return out


def resample_homography(src: torch.Tensor, resample_xf: torch.Tensor, out_hw: Tuple[int, int] = (arch.CROP, arch.CROP),
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ut_resample_homography.  src [n,H,W] u8 or f32, resample_xf [n,4,4] f32 -> [n,h,w] f32 in [0,1]."""
    lib = load_library()
    d = _hip_device(src, "resample_homography")
    if src.dim() != 3 or src.dtype not in (torch.uint8, torch.float32):
        raise ValueError("src must be [n,H,W] uint8 or float32")
    n = src.shape[0]
    xf = _need(resample_xf, torch.float32, d, "resample_xf").reshape(-1, 16)
    if xf.shape[0] != n:
        raise ValueError("resample_xf must hold one 4x4 matrix per source image")
    src = src.contiguous()
    out = _out(out, (n, out_hw[0], out_hw[1]), torch.float32, d, "out")
    with torch.cuda.device(d):
        rc = lib.ut_resample_homography(None, _ptr(src), int(src.dtype == torch.float32), n, src.shape[1], src.shape[2],
                                        _ptr(xf), out_hw[0], out_hw[1], _ptr(out), _stream(d))
    _check_rc(lib, None, rc, "ut_resample_homography")
    return out


def keypoint_metrics(gt: torch.Tensor, tracked: torch.Tensor, valid: torch.Tensor) -> Dict[str, torch.Tensor]:
    """ut_keypoint_metrics.  gt, tracked [hands, frames, 21, 3] f32, valid [hands, frames] bool/u8 on one HIP device ->
    err f64 [hands, frames], acc / gt_acc f64 [hands, frames-2], valid_acc bool [hands, frames-2]."""
    lib = load_library()
    d = _hip_device(gt, "keypoint_metrics")
    if gt.dim() != 4 or tuple(gt.shape[2:]) != (arch.N_LANDMARKS, 3) or gt.shape != tracked.shape:
        raise ValueError("gt and tracked must both be [hands, frames, 21, 3]")
    h, t = gt.shape[:2]
    if tuple(valid.shape) != (h, t):
        raise ValueError("valid must be [hands, frames]")
    g, p = _need(gt, torch.float32, d, "gt"), _need(tracked, torch.float32, d, "tracked")
    v = _need(valid, torch.uint8, d, "valid")
    ta = max(t - 2, 0)
    out = {"err": torch.empty(h, t, dtype=torch.float64, device=d), "acc": torch.empty(h, ta, dtype=torch.float64, device=d),
           "gt_acc": torch.empty(h, ta, dtype=torch.float64, device=d), "valid_acc": torch.zeros(h, ta, dtype=torch.uint8, device=d)}
    with torch.cuda.device(d):
        rc = lib.ut_keypoint_metrics(None, _ptr(g), _ptr(p), _ptr(v), h, t, _ptr(out["err"]), _ptr(out["acc"]),
                                     _ptr(out["gt_acc"]), _ptr(out["valid_acc"]), _stream(d))
    _check_rc(lib, None, rc, "ut_keypoint_metrics")
    out["valid_acc"] = out["valid_acc"].bool()
    return out


def warp_map(cam_params: torch.Tensor, crop_params: torch.Tensor, src_index: torch.Tensor, n_src_images: int) -> torch.Tensor:
    """ut_warp_map: the fp32 coordinate maps [n_crops,96,96,2] (x, y) the resampler samples with (what the reference hands to
    cv2.remap, lib/tracker/tracker.py:69-85)."""
    lib = load_library()
    d = _hip_device(cam_params, "warp_map")
    cam, crop = _need(cam_params, torch.float64, d, "cam_params"), _need(crop_params, torch.float64, d, "crop_params")
    idx = _need(src_index, torch.int32, d, "src_index")
    n = crop.shape[0]
    if crop.shape != (n, 24) or cam.dim() != 2 or cam.shape[1] != 32 or idx.shape != (n,) or cam.shape[0] < n_src_images:
        raise ValueError("cam_params [n_src,32] f64, crop_params [n,24] f64, src_index [n] i32")
    out = torch.empty(n, arch.CROP, arch.CROP, 2, device=d)
    with torch.cuda.device(d):
        rc = lib.ut_warp_map(_ptr(cam), _ptr(crop), _ptr(idx), int(n_src_images), n, _ptr(out), _stream(d))
    _check_rc(lib, None, rc, "ut_warp_map")
    return out


class HipEngine:
    """One native handle (packed weights + workspace + temporal state) on one GPU."""

    def __init__(self, state_dict, device="cuda"):
        if not torch.cuda.is_available():
            raise NativeLibraryError("no HIP device visible: the UmeTrack hot path has no CPU fallback")
        self.lib = load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NativeLibraryError(f"device {device!r} is not a HIP device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        blob = state_dict_to_blob(state_dict)
        h = ctypes.c_void_p()
        rc = self.lib.ut_create(self.device.index, blob.ctypes.data_as(ctypes.c_void_p), blob.size, ctypes.byref(h))
        _check_rc(self.lib, None, rc, "ut_create")
        self._h = h
        self.deferred_checks = False      # mirrors of the handle's modes (the C ABI has setters only)
        self.latency_mode = False
        self.split_scale = "calibrated"

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ut_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> int:
        return _check_rc(self.lib, self._h, rc, what, "engine")

    def set_index_checks(self, deferred: bool):
        """Default: every call that takes index tensors reads the device-side verdict back (one stream sync) and
        raises IndexError.  deferred=True: no sync (hipGraph capture, run-ahead launching); bad work is skipped on
        the device and `poll_status()` raises for it later."""
        self._check(self.lib.ut_set_index_checks(self._h, UT_CHECK_DEFERRED if deferred else UT_CHECK_SYNC),
                    "ut_set_index_checks")
        self.deferred_checks = bool(deferred)

    @contextlib.contextmanager
    def modes(self, deferred_checks: Optional[bool] = None, latency: Optional[bool] = None,
              split_scale: Optional[str] = None):
        """Switch the handle's check / latency / split-scale mode for the calls inside the `with` block and put back what
        was set before: a handle shared by a per-frame HandTracker (latency mode, deferred checks) and a batched HotPath
        keeps each user's settings out of the other's calls, and a HotPath user can scope e.g. split_scale="adaptive"."""
        prev = (self.deferred_checks, self.latency_mode, self.split_scale)
        try:
            if deferred_checks is not None and deferred_checks != prev[0]:
                self.set_index_checks(deferred_checks)
            if latency is not None and latency != prev[1]:
                self.set_latency_mode(latency)
            if split_scale is not None and split_scale != prev[2]:
                self.set_split_scale(split_scale)
            yield self
        finally:
            if self._h:
                if self.deferred_checks != prev[0]:
                    self.set_index_checks(prev[0])
                if self.latency_mode != prev[1]:
                    self.set_latency_mode(prev[1])
                if self.split_scale != prev[2]:
                    self.set_split_scale(prev[2])

    def status_snapshot(self, out: torch.Tensor):
        """Stream-ordered copy of the two device status words (sticky errors, this call's bits) into `out` (int32 [2] on
        the device) - for callers that read results back in one staged transfer and look at the verdict there."""
        out = _need(out, torch.int32, self.device, "out")
        self._check(self.lib.ut_status_snapshot(self._h, _ptr(out), _stream(self.device)), "ut_status_snapshot")

    def set_backbone_lanes(self, lanes: int):
        """2: large batches run as two half-batches on two internal streams (each fills the other's launch tails)."""
        self._check(self.lib.ut_set_backbone_lanes(self._h, int(lanes)), "ut_set_backbone_lanes")

    def set_block_fusion(self, on: bool):
        """Split-fp16 mode: layer1's BasicBlocks as one launch each (default) or as two convolution launches (A/B tests).  Both
        arithmetics: the fp32 1x1 convolutions (layer4's shortcut, the projection, the head's two chains) as streaming
        launches with the chains' intermediates in registers (default; same bits), or one conv_igemm launch per layer."""
        self._check(self.lib.ut_set_block_fusion(self._h, int(bool(on))), "ut_set_block_fusion")

    def set_resident_weights(self, kind=1):
        """Split-fp16 mode, A/B switch (include/umetrack_hip.h::ut_set_resident_weights): 1 / True (default) conv_w4.hip on the
        stride-1 convolutions of layer2 .. layer4 and the stride-2 entries of layer3 / layer4; 0 / False the chunked conv_split
        kernels everywhere; 6 as 1 but the stride-2 entries through the chunked gather kernel; and, with those through the gather
        kernel as well: 3 conv_w4 on all stride-1 convolutions, 2 conv_c64k.hip on layer2 and chunked elsewhere, 4 conv_w4 on
        layer3 / layer4 and conv_c64k on layer2, 5 conv_w4 on layer3 / layer4 and chunked on layer2.  In every kind the
        consecutive stride-1 convolutions that conv_w4 takes run as one launch per layer (a chain; calibrated scale mode, fusion
        switch on); 7 as 1 with one launch per convolution."""
        self._check(self.lib.ut_set_resident_weights(self._h, int(kind)), "ut_set_resident_weights")

    def set_latency_mode(self, on: bool):
        """Few-crop launches split K across workgroups (per-frame tracking); results then agree with the default mode to
        fp32 rounding instead of bit for bit.  Off by default."""
        self._check(self.lib.ut_set_latency_mode(self._h, int(bool(on))), "ut_set_latency_mode")
        self.latency_mode = bool(on)

    def set_conv_arithmetic(self, mode: str):
        """"fp32": exact fp32 matrix instructions (default).  "split_f16": the batched backbone convolutions run on the fp16
        matrix cores from two-piece splits of both operands (fp32-level error, not the fp32 chain's bits), for calls of
        >= 2 x CUs crops (one arithmetic per call); "split_f16_always": calls of any size (tests)."""
        self._check(self.lib.ut_set_conv_arithmetic(self._h, {"fp32": 0, "split_f16": 1, "split_f16_always": 2}[mode]), "ut_set_conv_arithmetic")

    def set_split_scale(self, mode: str):
        """Split-fp16 mode: "calibrated" (default) - one fixed power-of-two activation scale per backbone tensor and handle (a
        crop's bits do not depend on its batch, lane count or sharding; inputs beyond 32 x the calibration maximum are reported
        by poll_status as FloatingPointError) - or "dynamic": each launch scales by the largest magnitude its producer stored in
        this call - or "adaptive": calibrated, but a launch whose input lies outside the calibrated band (32 x the calibration
        maximum or more, or non-zero and below 2^-7 of it) runs exactly as in "dynamic" mode instead of raising or losing
        precision, and counts in split_adaptations().  In band its bits are the "calibrated" mode's.  The decision is per
        LAUNCH, made on the device: one dim crop in a normal batch stays in band (and keeps the calibrated floor).  Only an
        infinity or a NaN still raises."""
        self._check(self.lib.ut_set_split_scale(self._h, SPLIT_SCALE_MODES[mode]), "ut_set_split_scale")
        self.split_scale = mode

    def split_adaptations(self, reset: bool = False) -> int:
        """Split launches that adapted ("adaptive" split scale: input out of the calibrated band) since the counter was last
        reset; one count per launch, both lanes included.  Synchronises the current stream; reset=True zeroes the counter."""
        n = ctypes.c_uint32(0)
        self._check(self.lib.ut_get_split_adaptations(self._h, ctypes.byref(n), int(bool(reset)), _stream(self.device)),
                    "ut_get_split_adaptations")
        return int(n.value)

    def calibrate_split(self, crops: Optional[torch.Tensor] = None):
        """Take the calibrated activation scales from `crops` ([n,96,96] fp32 on the device; None: the built-in synthetic set,
        which is what a handle uses when this is never called)."""
        if crops is None:
            self._check(self.lib.ut_calibrate_split(self._h, None, 0, _stream(self.device)), "ut_calibrate_split")
            return
        crops = _need(crops, torch.float32, self.device, "crops")
        if crops.ndim != 3 or tuple(crops.shape[1:]) != (arch.CROP, arch.CROP) or crops.shape[0] == 0:
            raise ValueError(f"crops must be [n >= 1,{arch.CROP},{arch.CROP}], got {tuple(crops.shape)}")
        self._check(self.lib.ut_calibrate_split(self._h, _ptr(crops), crops.shape[0], _stream(self.device)), "ut_calibrate_split")

    def split_calibration(self) -> np.ndarray:
        """The 33 calibrated scale words (stem output, every block's inner tensor and output, 2 x 4 of the regressors) as float32."""
        out = np.zeros(33, np.float32)
        self._check(self.lib.ut_get_split_calibration(self._h, out.ctypes.data_as(ctypes.c_void_p)), "ut_get_split_calibration")
        return out

    def poll_status(self):
        self._check(self.lib.ut_poll_status(self._h, _stream(self.device)), "ut_poll_status")

    # ------------------------------------------------------------------ entry points
    def reserve(self, max_crops: int, max_samples: int, max_slots: int):
        self._check(self.lib.ut_reserve(self._h, max_crops, max_samples, max_slots), "ut_reserve")

    def set_backbone_chunk(self, crops: int):
        self._check(self.lib.ut_set_backbone_chunk(self._h, crops), "ut_set_backbone_chunk")

    def _warp(self, entry: str, out_shape, src_u8, cam_params, crop_params, src_index, mode, out):
        """ut_warp_crops / ut_warp_backbone: the same arguments, another output per crop."""
        d = self.device
        src_u8 = _need(src_u8, torch.uint8, d, "src")
        if src_u8.dim() != 3:
            raise ValueError("src must be [n_images, H, W] uint8")
        cam_params = _need(cam_params, torch.float64, d, "cam_params")
        crop_params = _need(crop_params, torch.float64, d, "crop_params")
        src_index = _need(src_index, torch.int32, d, "src_index")
        n = crop_params.shape[0]
        if cam_params.shape != (src_u8.shape[0], 32) or crop_params.shape != (n, 24) or src_index.shape != (n,):
            raise ValueError("bad cam_params / crop_params / src_index shape")
        if out is None:
            out = torch.empty(n, *out_shape, dtype=torch.float32, device=d)
        self._check(getattr(self.lib, entry)(self._h, _ptr(src_u8), src_u8.shape[0], src_u8.shape[1], src_u8.shape[2],
                                             _ptr(cam_params), _ptr(crop_params), _ptr(src_index), n, mode, _ptr(out),
                                             _stream(d)), entry)
        return out

    def warp_crops(self, src_u8: torch.Tensor, cam_params: torch.Tensor, crop_params: torch.Tensor,
                   src_index: torch.Tensor, mode: int = UT_REMAP_CV2_FIXED,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._warp("ut_warp_crops", (arch.CROP, arch.CROP), src_u8, cam_params, crop_params, src_index, mode, out)

    def warp_backbone(self, src_u8: torch.Tensor, cam_params: torch.Tensor, crop_params: torch.Tensor,
                      src_index: torch.Tensor, mode: int = UT_REMAP_CV2_FIXED,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ut_warp_backbone: resample + backbone with the crops kept in the handle's workspace (u8 in cv2 mode)."""
        return self._warp("ut_warp_backbone", (arch.FEAT_CH, arch.FEAT_HW, arch.FEAT_HW), src_u8, cam_params, crop_params,
                          src_index, mode, out)

    def backbone(self, crops: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        d = self.device
        crops = _need(crops, torch.float32, d, "crops")
        if crops.dim() != 3 or crops.shape[1:] != (arch.CROP, arch.CROP):
            raise ValueError(f"crops must be [n,96,96], got {tuple(crops.shape)}")
        n = crops.shape[0]
        if out is None:
            out = torch.empty(n, arch.FEAT_CH, arch.FEAT_HW, arch.FEAT_HW, dtype=torch.float32, device=d)
        self._check(self.lib.ut_backbone(self._h, _ptr(crops), n, _ptr(out), _stream(d)), "ut_backbone")
        return out

    def fuse_temporal_regress(self, feat, intrinsics, extrinsics, sample_range, memory_idx, use_memory, hand_idx,
                              n_slots: int, all_multiview: bool, skel: Optional[torch.Tensor], mode: int,
                              want_raw: bool = False, out: Optional[torch.Tensor] = None
                              ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        d = self.device
        feat = _need(feat, torch.float32, d, "feat")
        intrinsics = _need(intrinsics, torch.float32, d, "intrinsics")
        extrinsics = _need(extrinsics, torch.float32, d, "extrinsics")
        sample_range = _need(sample_range, torch.int64, d, "sample_range")
        memory_idx = _need(memory_idx, torch.int64, d, "memory_idx")
        hand_idx = _need(hand_idx, torch.int64, d, "hand_idx")
        use_memory = _need(use_memory.to(torch.uint8) if use_memory.dtype == torch.bool else use_memory,
                           torch.uint8, d, "use_memory")
        n, s = feat.shape[0], sample_range.shape[0]
        if intrinsics.shape != (n, 3, 3) or extrinsics.shape != (n, 4, 4) or sample_range.shape != (s, 2) \
                or memory_idx.shape != (s,) or use_memory.shape != (s,) or hand_idx.shape != (s,):
            raise ValueError("inconsistent frame data / frame desc shapes")
        n_skel = 0
        if skel is not None:
            skel = _need(skel, torch.float32, d, "skel")
            n_skel = skel.shape[0]
        if out is None:
            out = torch.empty(s, arch.POSE_REC, dtype=torch.float32, device=d)
        raw = torch.empty(s, 64, dtype=torch.float32, device=d) if want_raw else None
        self._check(self.lib.ut_fuse_temporal_regress(
            self._h, _ptr(feat), _ptr(intrinsics), _ptr(extrinsics), _ptr(sample_range), _ptr(memory_idx),
            _ptr(use_memory), _ptr(hand_idx), n, s, int(n_slots), int(bool(all_multiview)), _ptr(skel), n_skel, mode,
            _ptr(out), _ptr(raw), _stream(d)), "ut_fuse_temporal_regress")
        return out, raw

    def reset_memory(self):
        self._check(self.lib.ut_reset_memory(self._h), "ut_reset_memory")

    def get_memory(self, max_slots: int = 1 << 16):
        d = self.device
        n = self._check(self.lib.ut_get_memory(self._h, None, None, 0, _stream(d)), "ut_get_memory")
        n = min(n, max_slots)
        mem = torch.empty(n, arch.MEM_CH, arch.FEAT_HW, arch.FEAT_HW, dtype=torch.float32, device=d)
        ext = torch.empty(n, 4, 4, dtype=torch.float32, device=d)
        if n:
            self._check(self.lib.ut_get_memory(self._h, _ptr(mem), _ptr(ext), n, _stream(d)), "ut_get_memory")
        return mem, ext

    def fk(self, hand_model: torch.Tensor, joint_angles: torch.Tensor, wrist_xf: torch.Tensor,
           mirror: Optional[torch.Tensor] = None, t_scale: float = 1.0, ja_stride: int = 22, xf_stride: int = 16,
           n: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """hand_model [1|n,321]; joint_angles/wrist_xf either packed [n,22]/[n,4,4] or views into a pose
        record buffer with explicit strides (in floats)."""
        return _fk(self.lib, self._h, self.device, "engine", hand_model, joint_angles, wrist_xf, mirror, t_scale, ja_stride,
                   xf_stride, n, out)

    def profile_begin(self):
        self._check(self.lib.ut_profile_begin(self._h, _stream(self.device)), "ut_profile_begin")

    def profile_end_by_kind(self):
        """[(ms, launches, flops) of the fp32-matrix-instruction launches, (...) of the split-fp16 launches]"""
        ms, n, fl = (ctypes.c_double * 2)(), (ctypes.c_int64 * 2)(), (ctypes.c_double * 2)()
        self._check(self.lib.ut_profile_end_by_kind(self._h, _stream(self.device), ms, n, fl), "ut_profile_end_by_kind")
        return [(ms[k], n[k], fl[k]) for k in range(2)]

    def profile_end(self):
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        self._check(self.lib.ut_profile_end(self._h, _stream(self.device), ctypes.byref(ms), ctypes.byref(n),
                                            ctypes.byref(fl)), "ut_profile_end")
        return ms.value, n.value, fl.value
