"""Shared by tests/test_scale_host.py, tests/test_gpu_scale.py and tools/bench_scale.py: the numpy restatement of the pose fit
with a free hand scale (csrc/fit_scale.hip: ut_fit_pose_scale, ut_pool_scale), built on the functions of tests/fit_cases.py.
The reference calibrates a hand's scale only through its network; this restatement is the yardstick: dtype=np.float64 is the
oracle, dtype=np.float32 - the same code in float32 - says what float32 can give on the same data.

Scale s means hand.scaled_hand_model(model, s): joint_rest_positions and landmark_rest_positions times s.  The solver is the
one of fit_cases.fit with a 27th parameter sigma = ln s, ordered last: d landmark / d sigma = landmark - wrist translation
(every length of the hand grows about the wrist frame's origin), trial s_t = clamp(s exp(d sigma), SCALE_MIN, SCALE_MAX), and
the step-small rule also asks |d sigma| <= STEP_TOL.  After the loop the scale information of the accepted state: the Schur
complement of sigma in A + SCALE_INFO_LAMBDA D (A = J^T W J, D its floored diagonal), i.e. 1 / variance of ln s per unit^2 of
target noise once pose and wrist are marginalised.  The constants are those of csrc/fit_scale.hip."""
import numpy as np

import fit_cases as fc
import mesh_cases as mc

SCALE_MIN, SCALE_MAX = 0.25, 4.0
SCALE_INFO_LAMBDA = 1e-6
FREE, FIXED = 0, 1
CONVERGED, AT_MAX_ITERS, REFUSED, AT_BOUND = 1, 2, 4, 8
_FIELDS = ("joint_rotation_axes", "joint_rest_positions", "landmark_rest_positions", "landmark_rest_bone_weights",
           "landmark_rest_bone_indices")


def scaled_model(hm, s, dtype=np.float64):
    """The skeleton dict of hand.scaled_hand_model(hm, s) for s [B], one row per pose, rest positions multiplied in `dtype`
    (float32: the bits the kernel and scaled_hand_model produce)."""
    s = np.asarray(s).astype(dtype).reshape(-1)
    b = len(s)
    out = {k: np.broadcast_to(np.asarray(hm[k]), (b,) + np.asarray(hm[k]).shape[-2:]) for k in _FIELDS}
    for k in ("joint_rest_positions", "landmark_rest_positions"):
        out[k] = out[k].astype(dtype) * s[:, None, None]
    return out


def forward(hm, s, angles, eff_wrist, dtype=np.float64):
    """Landmarks [B,21,3] of the model scaled by s [B]: fit_cases.forward's arithmetic (frames of mesh_cases, (p, 1) times the
    dense weight first, frames summed in ascending order) with one set of rest positions per pose, without a loop over poses."""
    b = angles.shape[0]
    axes, rest, lm, dense = fc._model(hm, b, dtype)
    sc = np.asarray(s).astype(dtype).reshape(b, 1, 1)
    ja = np.zeros((b, 22), dtype)
    ja[:, :20] = angles[:, :20]
    frames = mc.skinning_frames(axes, rest * sc, ja, eff_wrist.astype(dtype))                   # [B,17,4,4]
    homo = np.concatenate([lm * sc, np.ones((b, 21, 1), dtype)], -1)                              # [B,21,4]
    return np.einsum("bfij,blfj->blfi", frames, homo[:, :, None, :] * dense[..., None]).sum(2)[..., :3]


def jacobian(hm, s, angles, eff_wrist, centroid, dtype=np.float64):
    """[B,63,27]: fit_cases.jacobian of the scaled model, and d landmarks / d ln s = landmark - wrist translation last."""
    b = angles.shape[0]
    jac = np.zeros((b, 63, 27), dtype)
    jac[:, :, :26] = fc.jacobian(scaled_model(hm, s, dtype), angles, eff_wrist, centroid, dtype)
    p = forward(hm, s, angles, eff_wrist, dtype)
    jac[:, :, 26] = (p - eff_wrist[:, None, :3, 3].astype(dtype)).reshape(b, 63)
    return jac


def trial_scale(s, d_sigma, dtype):
    """s_t = clamp(s exp(d sigma), SCALE_MIN, SCALE_MAX) in `dtype`."""
    dt = dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        st = np.minimum(np.maximum(s * np.exp(d_sigma), dt(SCALE_MIN)), dt(SCALE_MAX))
    return st.astype(dtype)


def apply_step(angles, eff_wrist, s, centroid, delta, box=None):
    """fit_cases.apply_step on the first 26 entries; s_t = clamp(s exp(delta[26]))."""
    a, m = fc.apply_step(angles, eff_wrist, centroid, delta[:, :26], box)
    return a, m, trial_scale(s, delta[:, 26], angles.dtype)


def information(a_mat, dtype=np.float64):
    """The scale information of normal matrices [B,27,27]: the Schur complement of the last parameter in
    A + SCALE_INFO_LAMBDA D - the square of the last pivot of its Cholesky factorisation, which is what the kernel computes.
    0 where that matrix is not positive definite."""
    dt = dtype
    diag = np.einsum("bii->bi", a_mat)
    diag = np.maximum(diag, dt(fc.DIAG_FLOOR) * diag.max(1, keepdims=True))
    m = (a_mat + np.einsum("bi,ij->bij", dt(SCALE_INFO_LAMBDA) * diag, np.eye(27, dtype=dt))).astype(dt)
    out = np.zeros(len(m), dt)
    for i in range(len(m)):
        try:
            np.linalg.cholesky(m[i, :26, :26])
            x = fc.solve(m[i, :26, :26], m[i, :26, 26])
            v = m[i, 26, 26] - m[i, 26, :26] @ x
            out[i] = v if np.isfinite(v) and v > 0 else 0
        except np.linalg.LinAlgError:
            pass
    return out


def _rows(hm, s, ang, m, centroid, w, used, y, mode, dt):
    """The weighted system (J [k,63,27], r [k,63]); mode FIXED: the sigma column is zero."""
    jac = jacobian(hm, s, ang, m, centroid, dt) * np.repeat(np.sqrt(w), 3, 1)[..., None]
    if mode == FIXED:
        jac[:, :, 26] = 0
    res = (np.where(used[..., None], forward(hm, s, ang, m, dt) - y, dt(0)) * np.sqrt(w)[..., None]).reshape(-1, 63)
    return jac, res


def _normal(hm, s, ang, m, centroid, w, used, y, mode, dt):
    jac, res = _rows(hm, s, ang, m, centroid, w, used, y, mode, dt)
    return jac.transpose(0, 2, 1) @ jac, (jac.transpose(0, 2, 1) @ res[..., None])[..., 0]


class _WithScale(fc.Problem):
    """fc.Problem with sigma = ln s as parameter 26: s [B] is the kept scale."""
    NP = 27

    def __init__(self, hm, dtype, w, used, y, refused, s, mode):
        super().__init__(hm, dtype, w, used, y, refused)
        self.s, self.mode = s, mode

    def model(self):
        return scaled_model(self.hm, self.s, self.dt)

    def system(self, idx, ang, m, centroid):
        return _rows(fc._take(self.hm, idx), self.s[idx], ang, m, centroid, self.w[idx], self.used[idx], self.y[idx], self.mode, self.dt)

    def cost(self, idx, ang, m, extra=None):
        s = self.s[idx] if extra is None else extra
        r = np.where(self.used[idx][..., None], forward(fc._take(self.hm, idx), s, ang, m, self.dt) - self.y[idx], self.dt(0))
        d2 = (r * r).sum(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            return (self.w[idx] * d2).sum(1), np.sqrt(d2.max(1))

    def trial(self, idx, delta):
        if self.mode == FIXED:
            delta[:, 26] = 0
        return trial_scale(self.s[idx], delta[:, 26], delta.dtype)

    def small(self, delta):
        return np.abs(delta[:, 26]) <= fc.STEP_TOL

    def keep(self, idx, accept, extra):
        self.s[idx[accept]] = extra[accept]

    def report(self, refused, ang, m, centroid, status):
        """The scale information of the accepted state and AT_BOUND, for a FREE fit; a refused pose's scale is 1."""
        scale_info = np.zeros(len(refused), self.dt)
        if self.mode == FREE and not refused.all():
            idx = np.nonzero(~refused)[0]
            jac, _res = self.system(idx, ang[idx], m[idx], centroid[idx])
            scale_info[idx] = information(jac.transpose(0, 2, 1) @ jac, self.dt)
            status[idx[(self.s[idx] <= self.dt(SCALE_MIN)) | (self.s[idx] >= self.dt(SCALE_MAX))]] |= AT_BOUND
        self.s[refused] = 1
        return [scale_info, np.zeros(len(refused), self.dt)]


def fit_scale(hm, targets, weights=None, limits=None, init=None, init_scale=None, mode=FREE, mirror=None, t_scale=1.0,
              max_iters=32, dtype=np.float64, trace=None):
    """fit_cases.fit with the scale: (joint_angles [B,22], wrist_xf [B,4,4], scale [B], info [B,6]: weighted rms residual,
    worst residual, iterations, status, scale information, 0).  init_scale [B] or None = 1; a non-finite one or one outside
    [SCALE_MIN, SCALE_MAX] refuses the pose (scale 1).  mode FIXED: the sigma column is zero, the scale stays init_scale and
    the information is 0.  Status bit AT_BOUND: a FREE fit ended at SCALE_MIN or SCALE_MAX.  trace: as for fit_cases.fit."""
    dt = dtype
    s = np.ones(targets.shape[0], dt) if init_scale is None else np.asarray(init_scale).astype(dt).copy()
    with np.errstate(invalid="ignore"):
        bad_scale = ~(np.isfinite(s) & (s >= dt(SCALE_MIN)) & (s <= dt(SCALE_MAX)))
    w, used, y, refused = fc.weighted_targets(targets, weights, dt, bad_scale)
    s[refused] = 1
    prob = _WithScale({k: np.asarray(hm[k]) for k in _FIELDS}, dt, w, used, y, refused, s, mode)
    out_ja, out_xf, info = fc.lm(prob, limits, init, mirror, t_scale, max_iters, trace=trace)
    return out_ja, out_xf, prob.s, info


def usable(scale, info):
    """The poses a pool uses: converged, neither refused nor at a bound, information finite and positive."""
    status = np.asarray(info)[:, 3].astype(np.int64)
    i = np.asarray(info)[:, 4].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ((status & CONVERGED) != 0) & ((status & (REFUSED | AT_BOUND)) == 0) & np.isfinite(i) & (i > 0)


def pool(scale, info, group_size):
    """ut_pool_scale in float64: [n_groups,4] = (scale = exp(sum I ln s / sum I), sigma = 1 / sqrt(sum I), scatter =
    sqrt(sum I (ln s - ln pooled)^2 / max(n_used - 1, 1)), n_used) over groups of group_size consecutive poses; a group
    without a usable pose gives (1, inf, 0, 0)."""
    scale, info = np.asarray(scale, np.float64), np.asarray(info, np.float64)
    n_groups = len(scale) // group_size
    out = np.zeros((n_groups, 4))
    ok = usable(scale, info)
    for g in range(n_groups):
        sl = slice(g * group_size, (g + 1) * group_size)
        use = ok[sl]
        if not use.any():
            out[g] = (1, np.inf, 0, 0)
            continue
        i, ls = info[sl, 4][use], np.log(scale[sl][use])
        mean = (i * ls).sum() / i.sum()
        out[g] = (np.exp(mean), 1 / np.sqrt(i.sum()), np.sqrt((i * (ls - mean) ** 2).sum() / max(use.sum() - 1, 1)), use.sum())
    return out
