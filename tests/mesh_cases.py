"""Shared by tests/test_mesh_host.py and tests/test_gpu_mesh.py: the mesh fixture, the poses the mesh tests run on and
the numpy oracle of the posed mesh.

The oracle restates lib/common/hand_skinning.py:17-186 (_skin_points) for any points and any dense [V,17] weight matrix:
 - `skin(..., np.float64)`: skinning frames by the algorithm of oracle/ref_fk.py (joint_local_xf, skinning_frames; that
   module casts to float32, so the float64 form is restated here and pinned against it by tests/test_mesh_host.py), a dense
   weighted sum over the 17 frames, area-weighted vertex normals;
 - `skin(..., np.float32)`: the same arithmetic in float32 with the frames taken from oracle.ref_fk.skinning_frames itself.
   Its distance to the float64 result is the yardstick of what float32 can give on this data.
"""
import os

import numpy as np

from oracle import ref_fk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_FRAMES = 17


def load_mesh(which: str):
    """(vertices f32 [V,3] mm, triangles i32 [T,3], dense_bone_weights f32 [V,17]); which = 'rec00' | 'generic'."""
    g = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))
    return g[which + ".mesh_vertices"], g[which + ".mesh_triangles"], g[which + ".dense_bone_weights"]


def label_poses(lab):
    """All 369 x 2 label poses of recording_00 as flat arrays: joint angles [738,22], wrist [738,4,4] (mm), hand [738]."""
    ja = lab["joint_angles"].reshape(-1, 22)
    xf = lab["wrist_transforms"].reshape(-1, 4, 4)
    hand = np.tile(np.arange(2), lab["joint_angles"].shape[0])
    return ja, xf, hand


def skeleton(npz, prefix):
    return {k[len(prefix):]: npz[k] for k in npz.files if k.startswith(prefix)}


def dense_landmark_weights(hm) -> np.ndarray:
    """[21,17] (hand_skinning.py:70-97: later non-zero entries overwrite)."""
    w, idx = np.asarray(hm["landmark_rest_bone_weights"]), np.asarray(hm["landmark_rest_bone_indices"]).astype(np.int64)
    dense = np.zeros((21, N_FRAMES), np.float32)
    for k in range(3):
        for l in range(21):
            if w[l, k] != 0:
                dense[l, idx[l, k]] = w[l, k]
    return dense


def _so3_exp(v, eps=1e-4):
    dt = v.dtype.type
    n2 = (v * v).sum(-1)
    theta = np.sqrt(np.maximum(n2, dt(eps)))
    inv = dt(1.0) / theta
    f1 = inv * np.sin(theta)
    f2 = inv * inv * (dt(1.0) - np.cos(theta))
    k = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    k[..., 0, 1], k[..., 0, 2] = -v[..., 2], v[..., 1]
    k[..., 1, 0], k[..., 1, 2] = v[..., 2], -v[..., 0]
    k[..., 2, 0], k[..., 2, 1] = -v[..., 1], v[..., 0]
    return f1[..., None, None] * k + f2[..., None, None] * (k @ k) + np.eye(3, dtype=v.dtype)


def skinning_frames(axes, rest, angles, wrist):
    """oracle/ref_fk.skinning_frames in the dtype of its inputs: [B,17,4,4]."""
    axes, rest, angles = axes[:, :20], rest[:, :20], angles[:, :20]
    r = _so3_exp(axes * angles[..., None])
    loc = np.zeros(angles.shape + (4, 4), angles.dtype)
    loc[..., :3, :3] = r
    loc[..., :3, 3] = rest - (r @ rest[..., None])[..., 0]
    loc[..., 3, 3] = 1
    frames = [wrist, wrist]
    for f in range(5):
        t = wrist
        for j in range(4):
            t = t @ loc[:, 4 * f + j]
            if j >= 1:
                frames.append(t)
    return np.stack(frames, 1)


def skin(hm, points, dense, joint_angles, wrist_xf, triangles=None, dtype=np.float64, mirror=None, t_scale=1.0):
    """Posed points [B,V,3] (and unit normals [B,V,3] when triangles are given).  hm: skeleton dict (joint_rotation_axes,
    joint_rest_positions, unbatched or [B,...]); mirror [B] of 0 / 1: column 0 of the wrist transform negated and the
    normals' sign flipped; the translation is multiplied by t_scale."""
    b = joint_angles.shape[0]
    ja = joint_angles.astype(dtype)
    xf = wrist_xf.astype(dtype).copy()
    xf[:, :3, 3] *= dtype(t_scale)
    if mirror is not None:
        xf[np.asarray(mirror) == 1, :, 0] *= -1
    axes = np.broadcast_to(np.asarray(hm["joint_rotation_axes"]).astype(dtype), (b, 22, 3))
    rest = np.broadcast_to(np.asarray(hm["joint_rest_positions"]).astype(dtype), (b, 22, 3))
    if dtype == np.float32:
        frames = ref_fk.skinning_frames(axes, rest, ja, xf)
        assert frames.dtype == np.float32
    else:
        frames = skinning_frames(axes, rest, ja, xf)
    homo = np.concatenate([points.astype(dtype), np.ones((points.shape[0], 1), dtype)], -1)       # [V,4]
    scaled = homo[:, None, :] * dense.astype(dtype)[:, :, None]                                   # [V,17,4]: (p,1) * w first
    out = np.empty((b, points.shape[0], 3), dtype)
    for lo in range(0, b, 64):
        per_frame = np.einsum("bfij,vfj->bvfi", frames[lo:lo + 64], scaled)                       # [b,V,17,4]
        out[lo:lo + 64] = per_frame.sum(2)[..., :3]
    if triangles is None:
        return out
    t = np.asarray(triangles).astype(np.int64)
    inc = np.zeros((points.shape[0], t.shape[0]), dtype)                                          # vertex x triangle incidence
    for k in range(3):
        np.add.at(inc, (t[:, k], np.arange(t.shape[0])), 1)
    nrm = np.empty_like(out)
    for lo in range(0, b, 64):
        p = out[lo:lo + 64]
        face = np.cross(p[:, t[:, 1]] - p[:, t[:, 0]], p[:, t[:, 2]] - p[:, t[:, 0]])             # [b,T,3], 2 x area x normal
        s = np.einsum("vt,btc->bvc", inc, face)
        length = np.sqrt((s * s).sum(-1, keepdims=True))
        nrm[lo:lo + 64] = np.where(length > 0, s / np.where(length > 0, length, 1), 0)
    if mirror is not None:
        nrm[np.asarray(mirror) == 1] *= -1
    return out, nrm


def signed_volume(p, triangles) -> np.ndarray:
    """[B] signed volume of the mesh p [B,V,3] measured from its centroid (the hand mesh is open at the wrist: the missing
    cap is a small cone from there); positive when the triangles are counter-clockwise seen from outside."""
    t = np.asarray(triangles).astype(np.int64)
    q = p.astype(np.float64) - p.astype(np.float64).mean(1, keepdims=True)
    return np.einsum("btc,btc->b", q[:, t[:, 0]], np.cross(q[:, t[:, 1]], q[:, t[:, 2]])) / 6.0
