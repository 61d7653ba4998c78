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


def apply_step(angles, eff_wrist, s, centroid, delta, box=None):
    """fit_cases.apply_step on the first 26 entries; s_t = clamp(s exp(delta[26]))."""
    dt = angles.dtype.type
    a, m = fc.apply_step(angles, eff_wrist, centroid, delta[:, :26], box)
    with np.errstate(over="ignore", invalid="ignore"):
        st = np.minimum(np.maximum(s * np.exp(delta[:, 26]), dt(SCALE_MIN)), dt(SCALE_MAX))
    return a, m, st.astype(angles.dtype)


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


def _normal(hm, s, ang, m, centroid, w, used, y, mode, dt):
    jac = jacobian(hm, s, ang, m, centroid, dt) * np.repeat(np.sqrt(w), 3, 1)[..., None]
    if mode == FIXED:
        jac[:, :, 26] = 0
    res = (np.where(used[..., None], forward(hm, s, ang, m, dt) - y, dt(0)) * np.sqrt(w)[..., None]).reshape(-1, 63)
    return jac.transpose(0, 2, 1) @ jac, (jac.transpose(0, 2, 1) @ res[..., None])[..., 0]


def fit_scale(hm, targets, weights=None, limits=None, init=None, init_scale=None, mode=FREE, mirror=None, t_scale=1.0,
              max_iters=32, dtype=np.float64, trace=None):
    """fit_cases.fit with the scale: (joint_angles [B,22], wrist_xf [B,4,4], scale [B], info [B,6]: weighted rms residual,
    worst residual, iterations, status, scale information, 0).  init_scale [B] or None = 1; a non-finite one or one outside
    [SCALE_MIN, SCALE_MAX] refuses the pose (scale 1).  mode FIXED: the sigma column is zero, the scale stays init_scale and
    the information is 0.  Status bit AT_BOUND: a FREE fit ended at SCALE_MIN or SCALE_MAX.  trace: as for fit_cases.fit."""
    dt = dtype
    b = targets.shape[0]
    hm = {k: np.asarray(hm[k]) for k in _FIELDS}
    w = np.ones((b, 21), dt) if weights is None else np.asarray(weights).astype(dt)
    used = w > 0
    s = np.ones(b, dt) if init_scale is None else np.asarray(init_scale).astype(dt).copy()
    with np.errstate(invalid="ignore"):
        bad_scale = ~(np.isfinite(s) & (s >= dt(SCALE_MIN)) & (s <= dt(SCALE_MAX)))
    refused = (used.sum(1) < 3) | ~np.isfinite(w).all(1) | (w < 0).any(1) | \
        (~np.isfinite(np.asarray(targets)) & used[..., None]).any((1, 2)) | bad_scale
    s[refused] = 1
    w = np.where(refused[:, None], dt(1), np.where(used, w, dt(0)))
    used = w > 0
    y = np.where(used[..., None], np.asarray(targets), 0).astype(dt)
    y[refused] = 0
    mir = np.zeros(b, np.int64) if mirror is None else np.asarray(mirror).astype(np.int64)
    box = None if limits is None else np.broadcast_to(np.asarray(limits).astype(dt)[..., :20, :], (b, 20, 2))
    wsum = w.sum(1)
    centroid = (w[..., None] * y).sum(1) / wsum[:, None]
    extent = np.sqrt((w * ((y - centroid[:, None]) ** 2).sum(-1)).sum(1) / wsum)
    tail = np.zeros((b, 2), dt)
    if init is None:
        ang, m = fc.cold_start(scaled_model(hm, s, dt), y, w, mir, box, dt)
    else:
        ang = np.asarray(init[0]).astype(dt)[:, :20].copy()
        tail = np.asarray(init[0]).astype(dt)[:, 20:22].copy()
        m = fc.effective_wrist(np.asarray(init[1]), mir, t_scale, dt)
        if box is not None:
            ang = np.minimum(np.maximum(ang, box[..., 0]), box[..., 1])

    def cost_of(a, mm, ss, sel):
        r = np.where(used[sel][..., None], forward(fc._take(hm, sel), ss, a, mm, dt) - y[sel], dt(0))
        d2 = (r * r).sum(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            return (w[sel] * d2).sum(1), np.sqrt(d2.max(1))

    every = np.arange(b)
    cost, worst = cost_of(ang, m, s, every)
    bad_start = ~refused & ~np.isfinite(cost)
    refused |= bad_start
    lam = np.full(b, fc.LAMBDA_START, dt)
    iters = np.zeros(b, np.int64)
    status = np.where(refused, REFUSED, 0)
    active = ~refused
    for _ in range(max_iters):
        if not active.any():
            break
        idx = np.nonzero(active)[0]
        sub = fc._take(hm, idx)
        a_mat, g = _normal(sub, s[idx], ang[idx], m[idx], centroid[idx], w[idx], used[idx], y[idx], mode, dt)
        diag = np.einsum("bii->bi", a_mat)
        diag = np.maximum(diag, dt(fc.DIAG_FLOOR) * diag.max(1, keepdims=True))
        damped = a_mat + np.einsum("bi,ij->bij", lam[idx, None] * diag, np.eye(27, dtype=dt))
        delta = fc.solve(damped, -g[..., None])[..., 0].astype(dt)
        ok = np.isfinite(delta).all(1)
        delta = np.where(ok[:, None], delta, 0)
        if mode == FIXED:
            delta[:, 26] = 0
        ta, tm, ts = apply_step(ang[idx], m[idx], s[idx], centroid[idx], delta, None if box is None else box[idx])
        tc, tw = cost_of(ta, tm, ts, idx)
        accept = ok & np.isfinite(tc) & (tc < cost[idx])
        if trace is not None:
            trace.append(fc.trial_record(idx, lam, delta, cost, tc, accept))
        step_small = (np.abs(ta - ang[idx]).max(1) <= fc.STEP_TOL) & (np.abs(delta[:, 20:23]).max(1) <= fc.STEP_TOL) & \
                     (np.abs(delta[:, 23:26]).max(1) <= dt(fc.STEP_TOL) * extent[idx]) & (np.abs(delta[:, 26]) <= fc.STEP_TOL)
        flat = ~accept | (cost[idx] - tc <= dt(fc.DECREASE_TOL) * cost[idx])
        with np.errstate(invalid="ignore"):
            stationary = ok & ~accept & (np.abs(tc - cost[idx]) <= dt(fc.FLAT_TOL) * cost[idx])
        done = (ok & step_small & flat & (lam[idx] <= fc.LAMBDA_CONVERGED_MAX)) | stationary
        acc = idx[accept]
        ang[acc], m[acc], s[acc], cost[acc], worst[acc] = ta[accept], tm[accept], ts[accept], tc[accept], tw[accept]
        lam[idx] = np.where(accept, np.maximum(lam[idx] * dt(fc.LAMBDA_DOWN), dt(fc.LAMBDA_MIN)), lam[idx] * dt(fc.LAMBDA_UP))
        iters[idx] += 1
        status[idx[done]] |= CONVERGED
        active[idx[done]] = False
    status[active] |= AT_MAX_ITERS
    fitted = ~refused
    scale_info = np.zeros(b, dt)
    if mode == FREE and fitted.any():
        idx = np.nonzero(fitted)[0]
        a_mat, _g = _normal(fc._take(hm, idx), s[idx], ang[idx], m[idx], centroid[idx], w[idx], used[idx], y[idx], mode, dt)
        scale_info[idx] = information(a_mat, dt)
        status[idx[(s[idx] <= dt(SCALE_MIN)) | (s[idx] >= dt(SCALE_MAX))]] |= AT_BOUND
    if box is None:
        big = np.abs(ang) > dt(np.pi)
        ang = np.where(big, fc.wrap(ang), ang)
    out_ja = np.concatenate([ang, tail], 1)
    out_xf = m.copy()
    out_xf[mir == 1, :, 0] *= -1
    out_xf[:, :3, 3] /= dt(t_scale)
    if refused.any():
        s[refused] = 1
        if init is None:
            out_ja[refused] = 0
            out_xf[refused] = np.eye(4, dtype=dt)
        else:
            out_ja[refused] = np.where(bad_start[refused, None], 0, np.asarray(init[0]).astype(dt)[refused])
            out_xf[refused] = np.where(bad_start[refused, None, None], np.eye(4), np.asarray(init[1]).astype(dt)[refused])
    info = np.stack([np.sqrt(cost / wsum), worst, iters.astype(dt), status.astype(dt), scale_info, np.zeros(b, dt)], 1)
    info[refused, :3] = 0
    return out_ja, out_xf, s, info


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
