"""Shared by the tests of the head past the backbone (test_head_math_host.py, test_gpu_head_edges.py,
test_gpu_split_range.py): the float64 head oracle fed given features, the Procrustes target families built from the
regressor's real source points, and the reference rotation computed two ways (their distance sizes the tolerances)."""
import numpy as np
import torch

from oracle import ref_model

ULP64 = 2.0 ** -52
ULP32 = 2.0 ** -23
# the head's tolerances against the float64 oracle (values as test_gpu_split_range.py introduced them)
FP32_TOL = 5e-6          # the exact-fp32 convolutions against fp64, relative to the reference's largest (max seen 2.23e-6)
ANGLE_TOL = 1e-4         # rad
METRE_TOL = 1e-6         # 1e-3 mm
RAW_TOL = 1.3e-6         # split regressor's raw outputs, relative to the largest (max seen 3.3e-7)


def head_oracle(sd64, feat, k, x, sr, mem_idx, use, hand, temporal, known, skel):
    """oracle.ref_model's head on `feat` (any dtype; run in float64): skel = (axes, rest), [22,3] each or [S,22,3] each."""
    fused = ref_model.fuse_views(sd64, feat.double(), k.double(), x.double(), sr)
    cam0 = x.double()[sr[:, 0]]
    t = temporal.step(sd64, fused, cam0, mem_idx, use)
    if known:
        s = ref_model.skeleton_features(sd64, *skel).expand(t.shape[0], -1, -1, -1)
        out = ref_model.regress(sd64, "_regressor_k", torch.cat([t, s], 1))
    else:
        out = ref_model.regress(sd64, "_regressor_u", t)
    out["wrist_xfs"] = ref_model.wrist_to_world(hand, cam0, out["wrist_xfs"])
    return out


def decode_reference(raw, known, hand, cam0_ext, dtype):
    """oracle.ref_model's decode (regress' slices, softplus, clamp, exp, procrustes, wrist_to_world) of raw outputs [S,>=d] in
    `dtype`."""
    name, d = ("_regressor_k", 62) if known else ("_regressor_u", 63)
    out = ref_model.decode(name, raw[:, :d].to(dtype))
    out["wrist_xfs"] = ref_model.wrist_to_world(hand, cam0_ext.to(dtype), out["wrist_xfs"])
    return out


def decode_errors(pose, raw, known, hand, cam0_ext):
    """decode_kernel in isolation: the pose record [S,60] against the float64 decode of the same raw [S,64], per output group.
    The bound is not the kernel's: the same decode in fp32 torch on the same raw is at distance D from the float64 one, and the
    kernel is allowed max(4 D, 4 fp32 ulp of the value) per element - absolute for angles, rotation entries and translations
    (D the group's largest), relative for the skeleton scale and the sigmas.
    {group: {"err": largest error, "dist": D, "ratio": largest error / allowance}}."""
    pose = pose.detach().cpu().double()
    raw = raw.detach().cpu().float()
    o64 = decode_reference(raw, known, hand, cam0_ext, torch.float64)
    o32 = decode_reference(raw, known, hand, cam0_ext, torch.float32)
    wrist = pose[:, 22:38].reshape(-1, 4, 4)
    groups = {"angles": (pose[:, :22], "joint_angles", None, False),
              "rotation": (wrist[:, :3, :3], "wrist_xfs", (slice(None), slice(0, 3), slice(0, 3)), False),
              "translation": (wrist[:, :3, 3], "wrist_xfs", (slice(None), slice(0, 3), 3), False),
              "sigmas": (pose[:, 39:60], "landmark_uncertainty_sigmas", None, True)}
    if not known:
        groups["scale"] = (pose[:, 38], "skel_scales", None, True)
    out = {}
    for g, (got, key, idx, relative) in groups.items():
        w64, w32 = (o64[key], o32[key].double()) if idx is None else (o64[key][idx], o32[key][idx].double())
        unit = w64.abs() if relative else torch.ones_like(w64)
        err, dist = (got - w64).abs() / unit, ((w32 - w64).abs() / unit).max()
        allow = torch.maximum(4 * dist, 4 * ULP32 * w64.abs() / unit)
        ok = allow > 0
        ratio = torch.where(ok, err / torch.where(ok, allow, torch.ones_like(allow)), torch.where(err > 0, torch.inf, 0.0))
        out[g] = {"err": err.max().item(), "dist": dist.item(), "ratio": ratio.max().item()}
    assert (wrist[:, 3] - torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).abs().max() <= 4 * ULP32
    return out


# ---------------------------------------------------------------- Procrustes inputs
def source_points() -> np.ndarray:
    """The regressor's seven source points as the kernel and the reference hold them: fp32 values, in float64."""
    return ref_model.rigid_source_points(torch.float32).double().numpy()


def rotations(rng, n, max_angle=np.pi) -> np.ndarray:
    """[n,3,3] proper rotations: uniform axis, angle uniform in [0, max_angle]."""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    th = rng.uniform(0.0, max_angle, n)[:, None, None]
    k = np.zeros((n, 3, 3))
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    k -= k.transpose(0, 2, 1)
    return np.eye(3)[None] + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def rigid4(rng, n, max_angle=np.pi, max_t=2.0) -> np.ndarray:
    """[n,4,4] float64 rigid transforms, rotations up to max_angle, translations U(-max_t, max_t)."""
    x = np.zeros((n, 4, 4))
    x[:, :3, :3] = rotations(rng, n, max_angle)
    x[:, :3, 3] = rng.uniform(-max_t, max_t, (n, 3))
    x[:, 3, 3] = 1.0
    return x


# target = (A (src * factors)) R^T + t with A a fixed rotation: A moves the scaling off the source's own symmetry axes (the source
# covariance has a repeated singular value, 0.0293 0.015 0.015), so that every family below has separated singular values
_A = rotations(np.random.default_rng(5), 1)[0]
WELL_POSED = {               # name -> factors; reflection expected for an odd number of negative ones
    "rigid": (1.0, 1.0, 1.0),
    "aniso": (1.3, 1.0, 0.6),
    "mirror_x": (-1.3, 1.0, 0.6),
    "mirror_y": (1.3, -1.0, 0.6),
    "mirror_z": (1.3, 1.0, -0.6),
    "third_+1e-7": (1.3, 1.0, 1e-7),
    "third_-1e-7": (1.3, 1.0, -1e-7),
    "coplanar": (1.3, 1.0, 0.0),
}
RANK_LE_1 = ("collinear", "coincident", "zero")


def targets(name, rng, n) -> np.ndarray:
    """[n,7,3] float64 target sets of one family (WELL_POSED, RANK_LE_1 or "random")."""
    src = source_points()
    r = rotations(rng, n)
    t = rng.uniform(-0.5, 0.5, (n, 1, 3))
    if name == "random":        # six decades of magnitude
        return rng.normal(size=(n, 7, 3)) * 10.0 ** rng.uniform(-4, 2, (n, 1, 1))
    if name == "collinear":
        return np.einsum("ij,nkj->nik", src * np.array([1.0, 0.0, 0.0]), r) + t
    if name == "coincident":
        return np.zeros((n, 7, 3)) + t
    if name == "zero":
        return np.zeros((n, 7, 3))
    base = src if name == "rigid" else (src @ _A.T) * np.array(WELL_POSED[name])
    return np.einsum("ij,nkj->nik", base, r) + t


def collinear_fp32() -> np.ndarray:
    """[7,3] collinear targets that stay collinear when rounded to fp32 (every coordinate a multiple of 2^-12 below 2): the
    source's x coordinates on a 2^-10 grid along (1/2, -1/4, 1) from (1/4, -1/2, 1)."""
    c = np.round(source_points()[:, 0] * 1024.0) / 1024.0
    dst = c[:, None] * np.array([0.5, -0.25, 1.0]) + np.array([0.25, -0.5, 1.0])
    assert (dst.astype(np.float32) == dst).all()
    return dst


def cross_covariance(dst) -> np.ndarray:
    """H [n,3,3] of oracle.ref_model.procrustes for the source points and targets dst [n,7,3]."""
    src = source_points()
    return np.einsum("ki,nkj->nij", src - src.mean(0), dst - dst.mean(1, keepdims=True))


def _rotation_from_svd(u, vt):
    v = np.swapaxes(vt, -1, -2)
    ut = np.swapaxes(u, -1, -2)
    w = np.zeros(u.shape)
    w[..., 0, 0] = w[..., 1, 1] = 1.0
    w[..., 2, 2] = np.linalg.det(v @ ut)
    return v @ w @ ut


def reference_rotation(h):
    """R = V diag(1, 1, det(V U^T)) U^T (lib/models/model_utils.py:40-49) in float64 from numpy's SVD of H, the same from the SVD
    of H^T (H^T = V S U^T), and the singular values: (R, R', s).  |R - R'| is the rounding the problem's conditioning lets through
    a float64 SVD - the yardstick a third float64 computation is held to."""
    u, s, vt = np.linalg.svd(h)
    u2, _s2, vt2 = np.linalg.svd(np.swapaxes(h, -1, -2))          # u2 = V, vt2 = U^T
    return _rotation_from_svd(u, vt), _rotation_from_svd(np.swapaxes(vt2, -1, -2), np.swapaxes(u2, -1, -2)), s


def rotation_defects(r):
    """(max |R R^T - I|, max |det R - 1|) of rotations [n,3,3]."""
    r = np.asarray(r, np.float64)
    return (np.abs(r @ np.swapaxes(r, -1, -2) - np.eye(3)).max(), np.abs(np.linalg.det(r) - 1.0).max())
