"""Shared by tests/test_fit_host.py, tests/test_gpu_fit.py and tools/bench_fit.py: the numpy restatement of the pose fit of
csrc/fit.hip (ut_fit_pose), the inverse of skin_landmarks.  The reference has no such solver, so this restatement is the
yardstick: `fit(..., dtype=np.float64)` is the oracle and `fit(..., dtype=np.float32)`, the same code in float32 (with numpy's
sgesv solve), says what float32 can give on the same data.

The forward function is the oracle of tests/mesh_cases.py (`skin` on the 21 landmark rest positions with
`dense_landmark_weights`).  The solver is Levenberg-Marquardt on 20 joint angles plus a wrist increment (rotation about the
weighted centroid of the targets, then translation): analytic Jacobian, Marquardt's diagonal scaling with a floor, a trial is
accepted only when the weighted cost goes down, cold start = rest pose + weighted Kabsch alignment of the rest landmarks.
The constants below are those of csrc/fit.hip."""
import numpy as np

import mesh_cases as mc

LAMBDA_START, LAMBDA_DOWN, LAMBDA_UP, LAMBDA_MIN = 1e-3, 0.1, 10.0, 1e-9
LAMBDA_CONVERGED_MAX = 1.0     # a small step under heavy damping is a stall, not convergence
DIAG_FLOOR = 1e-10             # relative to the largest diagonal entry of J^T W J
STEP_TOL = 1e-5                # rad for the angles and the wrist rotation; x the hand's extent for the translation
DECREASE_TOL = 1e-3            # relative cost decrease of the last accepted step
FLAT_TOL = 1e-6                # a rejected trial whose cost is the accepted one's to this relative distance: the cost is flat to
                               # float32 resolution across the step, nothing is left to gain (a stalled fit is rejected by more)
CONVERGED, AT_MAX_ITERS, REFUSED = 1, 2, 4


def wrap(a):
    """Angles into (-pi, pi]."""
    two_pi = a.dtype.type(2 * np.pi)
    return a - two_pi * np.ceil((a - a.dtype.type(np.pi)) / two_pi)


def angle_distance(a, b):
    """|a - b| modulo 2 pi, elementwise."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def _model(hm, b, dtype):
    axes = np.broadcast_to(np.asarray(hm["joint_rotation_axes"]).astype(dtype), (b, 22, 3))
    rest = np.broadcast_to(np.asarray(hm["joint_rest_positions"]).astype(dtype), (b, 22, 3))
    lm = np.asarray(hm["landmark_rest_positions"]).astype(dtype)
    if lm.ndim == 2:
        dense = np.broadcast_to(mc.dense_landmark_weights(hm).astype(dtype), (b, 21, 17))
    else:
        dense = np.stack([mc.dense_landmark_weights({k: np.asarray(v)[i] for k, v in hm.items()}) for i in range(b)]).astype(dtype)
    return axes, rest, np.broadcast_to(lm, (b, 21, 3)), dense


def _take(hm, idx):
    """Rows idx of a batched skeleton; an unbatched one as it is."""
    if np.asarray(hm["landmark_rest_positions"]).ndim == 2:
        return hm
    return {k: np.asarray(v)[idx] for k, v in hm.items()}


def effective_wrist(wrist_xf, mirror, t_scale, dtype):
    """The transform the skinning applies: translation times t_scale, column 0 negated where mirror == 1."""
    m = np.array(wrist_xf, dtype=dtype, copy=True)
    m[:, :3, 3] *= dtype(t_scale)
    if mirror is not None:
        m[np.asarray(mirror) == 1, :, 0] *= -1
    return m


def forward(hm, angles, eff_wrist, dtype=np.float64):
    """Landmarks [B,21,3] of 20 (or 22) angles and the effective wrist transform: mesh_cases.skin, one pose at a time when
    the skeleton is batched."""
    ja = np.zeros((angles.shape[0], 22), dtype)
    ja[:, :20] = angles[:, :20]
    lm = np.asarray(hm["landmark_rest_positions"])
    if lm.ndim == 2:
        return mc.skin(hm, lm, mc.dense_landmark_weights(hm), ja, eff_wrist, dtype=dtype)
    rows = [{k: np.asarray(v)[i] for k, v in hm.items()} for i in range(ja.shape[0])]
    return np.concatenate([mc.skin(r, r["landmark_rest_positions"], mc.dense_landmark_weights(r), ja[i:i + 1],
                                   eff_wrist[i:i + 1], dtype=dtype) for i, r in enumerate(rows)])


def jacobian(hm, angles, eff_wrist, centroid, dtype=np.float64):
    """d landmarks / d (20 angle increments, wrist rotation about `centroid`, wrist translation): [B,63,26], rows 3 l + d.
    Column k = 4 c + j sums over the frames of finger c that contain joint j (those after m = max(j, 1) .. 3 joints)
    w_lf * s * (omega x (T_f p_l - c_w)): omega = the prefix frame's linear part times the axis, c_w = the prefix frame
    applied to the joint's rest position, s = det of the wrist's linear part (-1 for mirrored poses).  The 1e-4 clamp of
    so3_exp_map is ignored."""
    b = angles.shape[0]
    axes, rest, lm, dense = _model(hm, b, dtype)
    r = mc._so3_exp(axes[:, :20] * angles[:, :20, None].astype(dtype))
    loc = np.zeros((b, 20, 4, 4), dtype)
    loc[..., :3, :3] = r
    loc[..., :3, 3] = rest[:, :20] - (r @ rest[:, :20, :, None])[..., 0]
    loc[..., 3, 3] = 1
    homo = np.concatenate([lm, np.ones((b, 21, 1), dtype)], -1)
    sign = np.sign(np.linalg.det(eff_wrist[:, :3, :3].astype(np.float64))).astype(dtype)
    jac = np.zeros((b, 21, 3, 26), dtype)
    for c in range(5):
        t = eff_wrist.astype(dtype)
        prefix, frames = [], {}
        for j in range(4):
            prefix.append(t)
            t = t @ loc[:, 4 * c + j]
            if j >= 1:
                frames[j] = t
        for j in range(4):
            omega = (prefix[j][:, :3, :3] @ axes[:, 4 * c + j, :, None])[..., 0]                         # [B,3]
            c_w = (prefix[j][:, :3, :3] @ rest[:, 4 * c + j, :, None])[..., 0] + prefix[j][:, :3, 3]     # [B,3]
            for m in range(max(j, 1), 4):
                y = np.einsum("bij,blj->bli", frames[m][:, :3, :], homo)                                 # [B,21,3]
                w = dense[:, :, 2 + 3 * c + m - 1]                                                       # [B,21]
                jac[:, :, :, 4 * c + j] += (w * sign[:, None])[..., None] * np.cross(omega[:, None, :], y - c_w[:, None, :])
    p = forward(hm, angles, eff_wrist, dtype)
    v = p - centroid[:, None, :]
    jac[:, :, 0, 21], jac[:, :, 0, 22] = v[..., 2], -v[..., 1]           # -hat(v)
    jac[:, :, 1, 20], jac[:, :, 1, 22] = -v[..., 2], v[..., 0]
    jac[:, :, 2, 20], jac[:, :, 2, 21] = v[..., 1], -v[..., 0]
    for d in range(3):
        jac[:, :, d, 23 + d] = 1
    return jac.reshape(b, 63, 26)


def _rodrigues(v):
    """exp(hat(v)), exact (no clamp), [B,3] -> [B,3,3]."""
    dt = v.dtype.type
    n2 = (v * v).sum(-1)
    small = n2 < dt(1e-8)
    th = np.sqrt(np.where(small, dt(1), n2))
    f1 = np.where(small, dt(1) - n2 / dt(6), np.sin(th) / th)
    f2 = np.where(small, dt(0.5) - n2 / dt(24), (dt(1) - np.cos(th)) / (th * th))
    k = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    k[..., 0, 1], k[..., 0, 2] = -v[..., 2], v[..., 1]
    k[..., 1, 0], k[..., 1, 2] = v[..., 2], -v[..., 0]
    k[..., 2, 0], k[..., 2, 1] = -v[..., 1], v[..., 0]
    return np.eye(3, dtype=v.dtype) + f1[..., None, None] * k + f2[..., None, None] * (k @ k)


def apply_step(angles, eff_wrist, centroid, delta, box=None):
    """The trial state of one step: angles + delta[:20] (clamped to the box), wrist <- rotation exp(delta[20:23]) about the
    centroid, then translation delta[23:26]."""
    a = angles + delta[:, :20]
    if box is not None:
        a = np.minimum(np.maximum(a, box[..., 0]), box[..., 1])
    e = _rodrigues(delta[:, 20:23])
    m = eff_wrist.copy()
    m[:, :3, :3] = e @ eff_wrist[:, :3, :3]
    m[:, :3, 3] = (e @ (eff_wrist[:, :3, 3] - centroid)[..., None])[..., 0] + centroid + delta[:, 23:26]
    return a, m


def kabsch(src, dst, w):
    """Weighted rigid alignment dst ~ R src + t: proper R [B,3,3], t [B,3]."""
    wn = w / w.sum(-1, keepdims=True)
    sc, dc = (wn[..., None] * src).sum(1), (wn[..., None] * dst).sum(1)
    h = np.einsum("bl,bli,blj->bij", w, src - sc[:, None], dst - dc[:, None]).astype(np.float64)
    u, _s, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.transpose(0, 2, 1) @ u.transpose(0, 2, 1)))
    fix = np.tile(np.eye(3), (len(h), 1, 1))
    fix[:, 2, 2] = d
    r = (vt.transpose(0, 2, 1) @ fix @ u.transpose(0, 2, 1)).astype(src.dtype)
    return r, dc - (r @ sc[..., None])[..., 0]


def cold_start(hm, targets, weights, mirror, box=None, dtype=np.float64):
    """Where a fit without an init starts: (angles [B,20] = the rest pose clamped to the box, effective wrist [B,4,4] =
    the weighted Kabsch alignment of that pose's landmarks to the targets, times the mirror)."""
    b = targets.shape[0]
    ang = np.zeros((b, 20), dtype)
    if box is not None:
        ang = np.minimum(np.maximum(ang, box[..., 0]), box[..., 1]).astype(dtype)
    flip = np.where(np.asarray(mirror) == 1, -1, 1).astype(dtype)
    eye = np.tile(np.eye(4, dtype=dtype), (b, 1, 1))
    eye[:, 0, 0] = flip
    r, t = kabsch(forward(hm, ang, eye, dtype), targets.astype(dtype), weights.astype(dtype))
    m = np.tile(np.eye(4, dtype=dtype), (b, 1, 1))
    m[:, :3, :3] = r
    m[:, :3, 0] *= flip[:, None]                                # R diag(s, 1, 1)
    m[:, :3, 3] = t
    return ang, m


def solve(a, b):
    """The linear solve of a step, (A + lambda D) delta = -g, and of scale_cases.information.  A function of its own so that a
    test can put another float32 algorithm in its place (step_cases.cholesky_solve): two correct float32 solvers differ by what
    rounding alone does."""
    return np.linalg.solve(a, b)


def trial_record(idx, lam, delta, cost, trial_cost, accept):
    """What `trace` receives per iteration, for the poses `idx` still active in it: the damping the step was solved with,
    the step before the box clamps it, the accepted cost it started from, the trial's cost and the decision."""
    return dict(idx=idx.copy(), lam=lam[idx].copy(), delta=delta.copy(), cost=cost[idx].copy(), trial_cost=trial_cost.copy(),
                accept=accept.copy())


def weighted_targets(targets, weights, dtype, also_refused=False):
    """The targets as `fit` and scale_cases.fit_scale read them: (w [B,21], 0 where unused and 1 for refused poses; used = w > 0;
    y [B,21,3], 0 where unused; refused [B]: fewer than 3 weighted landmarks, a negative or non-finite weight, a non-finite
    target of a weighted landmark, or `also_refused`)."""
    dt = dtype
    w = np.ones((targets.shape[0], 21), dt) if weights is None else np.asarray(weights).astype(dt)
    used = w > 0
    refused = (used.sum(1) < 3) | ~np.isfinite(w).all(1) | (w < 0).any(1) | \
        (~np.isfinite(np.asarray(targets)) & used[..., None]).any((1, 2)) | also_refused
    w = np.where(refused[:, None], dt(1), np.where(used, w, dt(0)))
    used = w > 0
    y = np.where(used[..., None], np.asarray(targets), 0).astype(dt)
    y[refused] = 0
    return w, used, y, refused


class Problem:
    """A cost as the loop `lm` sees it, shaped like the problem P of csrc/ut_fit_dev.h.  As it stands it is `fit`'s: the
    weighted distance to 3-D targets (hm; dt the working dtype; w, used, y, refused of weighted_targets).  The other
    restatements derive from it and replace what differs; `idx` are the poses still active, states are theirs alone.
      NP                              the parameter count: 20 angles, the wrist increment, then the problem's own
      model()                         the skeleton the cold start poses
      cold_start(mir, box)            (angles [B,20], effective wrist [B,4,4]) where a fit without an init starts
      pivot(ang, m)                   (centroid [B,3] the wrist increment turns about, extent [B] that scales the translation's
                                      step tolerance, the denominator [B] of info's rms) - of the start ang, m or of the targets
      system(idx, ang, m, centroid)   the linearised system (J [k,63,NP], r [k,63]) in dt
      cost(idx, ang, m, extra=None)   (cost [k], worst residual [k]) of a state; extra: a trial's own state in place of the kept
      trial(idx, delta)               a trial's state beyond angles and wrist (None: there is none); it may edit delta first
      small(delta)                    what else the step-small rule asks
      keep(idx, accept, extra)        an accepted trial's own state becomes the kept one
      report(refused, ang, m, centroid, status)   after the loop: columns of info beyond the four, status bits of its own"""
    NP = 26

    def __init__(self, hm, dtype, w, used, y, refused):
        self.hm, self.dt, self.w, self.used, self.y, self.refused = hm, dtype, w, used, y, refused

    def model(self):
        return self.hm

    def cold_start(self, mir, box):
        return cold_start(self.model(), self.y, self.w, mir, box, self.dt)

    def pivot(self, ang, m):
        wsum = self.w.sum(1)
        centroid = (self.w[..., None] * self.y).sum(1) / wsum[:, None]
        extent = np.sqrt((self.w * ((self.y - centroid[:, None]) ** 2).sum(-1)).sum(1) / wsum)
        return centroid, extent, wsum

    def system(self, idx, ang, m, centroid):
        sub, dt, root = _take(self.hm, idx), self.dt, np.sqrt(self.w[idx])
        jac = jacobian(sub, ang, m, centroid, dt) * np.repeat(root, 3, 1)[..., None]
        res = (np.where(self.used[idx][..., None], forward(sub, ang, m, dt) - self.y[idx], dt(0)) * root[..., None]).reshape(-1, 63)
        return jac, res

    def cost(self, idx, ang, m, extra=None):
        r = np.where(self.used[idx][..., None], forward(_take(self.hm, idx), ang, m, self.dt) - self.y[idx], self.dt(0))
        d2 = (r * r).sum(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            return (self.w[idx] * d2).sum(1), np.sqrt(d2.max(1))

    def trial(self, idx, delta):
        return None

    def small(self, delta):
        return True

    def keep(self, idx, accept, extra):
        pass

    def report(self, refused, ang, m, centroid, status):
        return []


def lm(prob, limits, init, mirror, t_scale, max_iters, history=None, trace=None):
    """The restatement of fit_pose (csrc/ut_fit_dev.h) on a Problem, once for all four entries.  Prologue: mirror flags, the box,
    the start - init = (joint_angles [B,22], wrist_xf [B,4,4]) clamped into the box, or the problem's cold start - the pivot, the
    start's cost; a start whose cost is not finite is refused.  Loop: Marquardt's floored diagonal scaling, the damped solve
    through `solve`, a trial kept only when the cost goes down, the stop rules and the lambda schedule.  Epilogue: angles
    wrapped into (-pi, pi] without a box, the proper wrist in target units / t_scale, a refused pose gets its init back (the
    rest pose at the identity without one or after a bad start).  Returns (joint_angles [B,22], wrist_xf [B,4,4], info
    [B, 4 + the problem's columns]: rms, worst, iterations, status - zeros before the status of a refused pose)."""
    dt = prob.dt
    refused = prob.refused.copy()
    b = len(refused)
    mir = np.zeros(b, np.int64) if mirror is None else np.asarray(mirror).astype(np.int64)
    box = None if limits is None else np.broadcast_to(np.asarray(limits).astype(dt)[..., :20, :], (b, 20, 2))
    tail = np.zeros((b, 2), dt)
    if init is None:
        ang, m = prob.cold_start(mir, box)
    else:
        ang = np.asarray(init[0]).astype(dt)[:, :20].copy()
        tail = np.asarray(init[0]).astype(dt)[:, 20:22].copy()
        m = effective_wrist(np.asarray(init[1]), mir, t_scale, dt)
        if box is not None:
            ang = np.minimum(np.maximum(ang, box[..., 0]), box[..., 1])
    centroid, extent, denominator = prob.pivot(ang, m)
    cost, worst = prob.cost(np.arange(b), ang, m)
    bad_start = ~refused & ~np.isfinite(cost)
    refused |= bad_start
    lam = np.full(b, LAMBDA_START, dt)
    iters = np.zeros(b, np.int64)
    status = np.where(refused, REFUSED, 0)
    active = ~refused
    for _ in range(max_iters):
        if not active.any():
            break
        idx = np.nonzero(active)[0]
        jac, res = prob.system(idx, ang[idx], m[idx], centroid[idx])
        a_mat = jac.transpose(0, 2, 1) @ jac
        g = (jac.transpose(0, 2, 1) @ res[..., None])[..., 0]
        diag = np.einsum("bii->bi", a_mat)
        diag = np.maximum(diag, dt(DIAG_FLOOR) * diag.max(1, keepdims=True))
        damped = a_mat + np.einsum("bi,ij->bij", lam[idx, None] * diag, np.eye(prob.NP, dtype=dt))
        delta = solve(damped, -g[..., None])[..., 0].astype(dt)
        ok = np.isfinite(delta).all(1)
        delta = np.where(ok[:, None], delta, 0)
        extra = prob.trial(idx, delta)
        ta, tm = apply_step(ang[idx], m[idx], centroid[idx], delta[:, :26], None if box is None else box[idx])
        tc, tw = prob.cost(idx, ta, tm, extra)
        accept = ok & np.isfinite(tc) & (tc < cost[idx])
        if trace is not None:
            trace.append(trial_record(idx, lam, delta, cost, tc, accept))
        step_small = (np.abs(ta - ang[idx]).max(1) <= STEP_TOL) & (np.abs(delta[:, 20:23]).max(1) <= STEP_TOL) & \
                     (np.abs(delta[:, 23:26]).max(1) <= dt(STEP_TOL) * extent[idx]) & prob.small(delta)
        with np.errstate(invalid="ignore"):
            flat = ~accept | (cost[idx] - tc <= dt(DECREASE_TOL) * cost[idx])
            stationary = ok & ~accept & (np.abs(tc - cost[idx]) <= dt(FLAT_TOL) * cost[idx])
        done = (ok & step_small & flat & (lam[idx] <= LAMBDA_CONVERGED_MAX)) | stationary
        acc = idx[accept]
        ang[acc], m[acc], cost[acc], worst[acc] = ta[accept], tm[accept], tc[accept], tw[accept]
        prob.keep(idx, accept, extra)
        lam[idx] = np.where(accept, np.maximum(lam[idx] * dt(LAMBDA_DOWN), dt(LAMBDA_MIN)), lam[idx] * dt(LAMBDA_UP))
        iters[idx] += 1
        status[idx[done]] |= CONVERGED
        active[idx[done]] = False
        if history is not None:
            history.append((ang.copy(), m.copy()))
    status[active] |= AT_MAX_ITERS
    columns = prob.report(refused, ang, m, centroid, status)
    if box is None:
        big = np.abs(ang) > dt(np.pi)
        ang = np.where(big, wrap(ang), ang)
    out_ja = np.concatenate([ang, tail], 1)
    out_xf = m.copy()
    out_xf[mir == 1, :, 0] *= -1
    out_xf[:, :3, 3] /= dt(t_scale)
    if refused.any():
        if init is None:
            out_ja[refused] = 0
            out_xf[refused] = np.eye(4, dtype=dt)
        else:
            out_ja[refused] = np.where(bad_start[refused, None], 0, np.asarray(init[0]).astype(dt)[refused])
            out_xf[refused] = np.where(bad_start[refused, None, None], np.eye(4), np.asarray(init[1]).astype(dt)[refused])
    with np.errstate(invalid="ignore"):
        info = np.stack([np.sqrt(cost / denominator), worst, iters.astype(dt), status.astype(dt)] + columns, 1)
    info[refused, :3] = 0
    return out_ja, out_xf, info


def fit(hm, targets, weights=None, limits=None, init=None, mirror=None, t_scale=1.0, max_iters=32, dtype=np.float64,
        history=None, trace=None):
    """Fit B poses: (joint_angles [B,22], wrist_xf [B,4,4] proper, translation in target units / t_scale, info [B,4]:
    weighted rms residual, worst residual, iterations, status).  targets [B,21,3]; weights [B,21] >= 0 or None; limits
    [20,2] / [B,20,2] or None; init = (joint_angles [B,22], wrist_xf [B,4,4]) or None for the cold start; mirror [B] of
    0 / 1.  history: a list that receives (angles, effective wrist) after every iteration.  trace: a list that receives
    the decision of every iteration (trial_record)."""
    return lm(Problem(hm, dtype, *weighted_targets(targets, weights, dtype)), limits, init, mirror, t_scale, max_iters, history, trace)


