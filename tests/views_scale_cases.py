"""Shared by tests/test_views_scale_host.py, tests/test_gpu_views_scale.py and tools/bench_views_scale.py: the numpy restatement
of ut_fit_pose_views_scale (include/umetrack_hip_views_scale.h, csrc/fit_views_scale.hip) and the cases its tests share.

The restatement is an fc.Problem with NP = 27 composed from what exists: the observations, the per-landmark blocks and the
semidefinite 3 x 3 Cholesky of views_cases (with the loss of robust_cases), ic.whiten, and the scale's trial, step rule,
information, bounds and AT_BOUND of scale_cases, under the loop fc.lm.  It takes the kernel's decisions: scale s means
scale_cases.scaled_model(hm, s) in the working dtype; d landmark / d sigma = landmark - wrist translation is column 26 of the
landmark's three rows BEFORE the whitening L^T a, and stays zero when the scale is fixed; the refusals are those of
views_cases.Views plus a start scale that is not finite or lies outside [SCALE_MIN, SCALE_MAX]; a refused pose has scale 1 and
information 0.  `dtype=np.float64` is the oracle, `dtype=np.float32` the same code in float32 with numpy's LU solve or
step_cases.cholesky_solve (`solver`)."""
import functools

import numpy as np

import fit_cases as fc
import info_cases as ic
import robust_cases as rc
import scale_cases as sc
import step_cases as st
import triangulate_cases as tc
import views_cases as vc

FREE, FIXED = sc.FREE, sc.FIXED
CONVERGED, AT_MAX_ITERS, REFUSED, AT_BOUND = sc.CONVERGED, sc.AT_MAX_ITERS, sc.REFUSED, sc.AT_BOUND
SCALE_TOL, INFO_RTOL = 4e-6, 1e-3          # the values of tests/test_gpu_scale.py


# ----------------------------------------------------------------------------- the linearised systems
def reduced_system(vw, hm, s, ang, m, centroid, idx, mode, dtype):
    """The 63 rows the solver sees for poses idx at scales s [k]: (J [k,63,27], r [k,63]) in dtype.  Column 26 is landmark - wrist
    translation (zero when mode is FIXED), written before the landmark's rows a are replaced by L^T a."""
    k = len(idx)
    sub = sc.scaled_model(fc._take(hm, idx), s, dtype)
    p = fc.forward(sub, ang, m, dtype)
    _c, mm, g, _good, _sq, _r, _j = vw.blocks(p, idx)
    f, rho = vc.semidefinite_cholesky(mm, g)
    any_used = vw.used[idx].any(1)
    f = np.where(any_used[..., None], f, 0.0).astype(dtype)
    rho = np.where(any_used[..., None], rho, 0.0).astype(dtype)
    jac = np.zeros((k, 21, 3, 27), dtype)
    jac[..., :26] = fc.jacobian(sub, ang, m, centroid, dtype).reshape(k, 21, 3, 26)
    if mode == FREE:
        jac[..., 26] = p - m[:, None, :3, 3].astype(dtype)
    jac = ic.whiten(f, np.where(any_used[..., None, None], jac, dtype(0))).reshape(k, 63, 27)
    return jac, rho.reshape(k, 63)


def stacked_system(vw, hm, s, ang, m, centroid, idx):
    """The full Gauss-Newton system in float64, 2 V 21 rows: (J [k,V*21*2,27], r [k,V*21*2]), rows weighted by sqrt(w psi); the
    sigma column is J_v (p - t) per view."""
    k = len(idx)
    sub = sc.scaled_model(fc._take(hm, idx), s, np.float64)
    p = fc.forward(sub, ang, m, np.float64)
    _c, _m, _g, _good, sq, res, jacs = vw.blocks(p, idx)
    jl = np.zeros((k, 21, 3, 27))
    jl[..., :26] = fc.jacobian(sub, ang, m, centroid, np.float64).reshape(k, 21, 3, 26)
    jl[..., 26] = p - m[:, None, :3, 3]
    rows_j, rows_r = [], []
    for v in range(vw.v_max):
        sw = np.sqrt(vw.w[idx, v] * rc.psi(vw.loss, sq[:, v], vw.loss_scale))
        rows_j.append((sw[..., None, None] * (jacs[v] @ jl)).reshape(k, 42, 27))
        rows_r.append((sw[..., None] * res[v]).reshape(k, 42))
    return np.concatenate(rows_j, 1), np.concatenate(rows_r, 1)


# ----------------------------------------------------------------------------- the fit
class _ReprojectionScale(fc.Problem):
    """fc.Problem on the observations vw (rc.RobustViews) with sigma = ln s as parameter 26: s [B] is the kept scale.  residual
    [B,V,21] float32 and inlier [B,V,21] float64 after the fit."""
    NP = 27

    def __init__(self, hm, dtype, vw, s, mode):
        self.hm, self.dt, self.vw, self.refused, self.s, self.mode = hm, dtype, vw, vw.refused, s, mode

    def landmarks(self, idx, s, ang, m):
        return fc.forward(sc.scaled_model(fc._take(self.hm, idx), s, self.dt), ang, m, self.dt)

    def _cost(self, idx, s, ang, m):
        with np.errstate(all="ignore"):
            return self.vw.cost(self.landmarks(idx, s, ang, m), idx, self.dt)

    def pivot(self, ang, m):
        with np.errstate(all="ignore"):
            return vc.pivot(self.vw, self.landmarks(np.arange(len(self.s)), self.s, ang, m), self.dt)

    def system(self, idx, ang, m, centroid):
        return reduced_system(self.vw, self.hm, self.s[idx], ang, m, centroid, idx, self.mode, self.dt)

    def cost(self, idx, ang, m, extra=None):
        return self._cost(idx, self.s[idx] if extra is None else extra, ang, m)[:2]

    def trial(self, idx, delta):
        if self.mode == FIXED:
            delta[:, 26] = 0
        return sc.trial_scale(self.s[idx], delta[:, 26], delta.dtype)

    def small(self, delta):
        return np.abs(delta[:, 26]) <= fc.STEP_TOL

    def keep(self, idx, accept, extra):
        self.s[idx[accept]] = extra[accept]

    def report(self, refused, ang, m, centroid, status):
        every = np.arange(len(refused))
        scale_info = np.zeros(len(refused), self.dt)
        if self.mode == FREE and not refused.all():
            idx = np.nonzero(~refused)[0]
            jac, _res = self.system(idx, ang[idx], m[idx], centroid[idx])
            scale_info[idx] = sc.information(jac.transpose(0, 2, 1) @ jac, self.dt)
            status[idx[(self.s[idx] <= self.dt(sc.SCALE_MIN)) | (self.s[idx] >= self.dt(sc.SCALE_MAX))]] |= AT_BOUND
        with np.errstate(all="ignore"):
            p = self.landmarks(every, self.s, ang, m)
            residual = self.vw.cost(p, every, self.dt)[2]
            psi_end = self.vw.inliers(p, every)
        self.residual = np.where(refused[:, None, None], 0.0, residual).astype(np.float32)
        self.inlier = np.where(refused[:, None, None], 0.0, psi_end)
        self.s[refused] = 1
        return [scale_info, np.zeros(len(refused), self.dt)]


def fit_views_scale(hm, window, cam_rows, table, weights=None, init=None, init_scale=None, mode=FREE, mirror=None, limits=None,
                    t_scale=1.0, max_iters=32, loss="squared", loss_scale=3.0, dtype=np.float64, solver="lu", trace=None):
    """ut_fit_pose_views_scale: (joint_angles [B,22], wrist_xf [B,4,4], scale [B], info [B,6]: sqrt(cost / sum of the used
    weights), the largest raw reprojection distance, iterations, status, scale information, 0; residual [B,V,21]; inlier
    [B,V,21]).  init is required.  init_scale [B] or None = 1; a non-finite one or one outside [SCALE_MIN, SCALE_MAX] refuses the
    pose (scale 1, the start comes back)."""
    if init is None:
        raise ValueError("init is required: there is no cold start")
    dt = dtype
    vw = rc.RobustViews(window, cam_rows, table, weights, dt, loss, loss_scale)
    s = np.ones(len(vw.refused), dt) if init_scale is None else np.asarray(init_scale).astype(dt).copy()
    with np.errstate(invalid="ignore"):
        bad_scale = ~(np.isfinite(s) & (s >= dt(sc.SCALE_MIN)) & (s <= dt(sc.SCALE_MAX)))
    vw.refused = vw.refused | bad_scale
    s[vw.refused] = 1
    prob = _ReprojectionScale({k: np.asarray(hm[k]) for k in sc._FIELDS}, dt, vw, s, mode)
    with st.solver(solver):
        ja, xf, info = fc.lm(prob, limits, init, mirror, t_scale, max_iters, trace=trace)
    return ja, xf, prob.s, info, prob.residual, prob.inlier


# ----------------------------------------------------------------------------- cases
SCALES = (0.8, 1.25)
STEP_CASES = ("two_views", "pinhole", "metres", "ragged")


@functools.lru_cache(maxsize=None)
def case(name, k, loss="squared", loss_scale=rc.SCALE_PX):
    """views_cases.case(name) with the exact windows of the label poses on the case's skeleton scaled by k: the starts are
    views_cases.case's (+-0.2 rad / +-15 mm, seed 31), the start scale is 1, mode FREE; truth = the float64 landmarks behind the
    windows, true_scale = k.  `ragged` is views_cases.ragged of the two-view case.  Cached: leave it unchanged."""
    base = vc.case("two_views" if name == "ragged" else name)
    truth = vc.posed(vc.golden(), sc.scaled_model(base["hm"], np.full(len(base["mirror"]), k)))
    c = dict(base, window=vc.exact_windows(base["table"], base["cam_rows"], truth), truth=truth)
    if name == "ragged":
        c = vc.ragged(c)
    c.update(init_scale=np.ones(len(c["mirror"]), np.float32), mode=FREE, true_scale=k, loss=loss, loss_scale=loss_scale)
    return c


def subset(c, sel):
    out = rc.subset(c, sel)
    out["init_scale"] = np.asarray(c["init_scale"])[np.asarray(sel)]
    return out


def restate(c, dtype=np.float64, max_iters=1, solver="lu", trace=None):
    """fit_views_scale on a case: dict(ja, xf, scale, info, residual, inlier)."""
    out = fit_views_scale(c["hm"], c["window"], c["cam_rows"], c["table"], c["weights"], c["init"], c["init_scale"], c["mode"],
                          c["mirror"], c["limits"], c["t_scale"], max_iters, c["loss"], c["loss_scale"], dtype, solver, trace)
    return dict(zip(("ja", "xf", "scale", "info", "residual", "inlier"), out))


def landmarks(c, res):
    """The float64 forward function of a result on the case's skeleton at the result's scale, in the cameras' world."""
    m = fc.effective_wrist(np.asarray(res["xf"], np.float64), c["mirror"], c["t_scale"], np.float64)
    hm = sc.scaled_model(c["hm"], np.asarray(res["scale"], np.float64))
    return fc.forward(hm, np.asarray(res["ja"], np.float64)[:, :20], m, np.float64)


def distance(c, a, b):
    """How far two results of a case lie apart: views_cases.distance's ang (rad), kp (mm, each result at its own scale) and px
    (rms / worst of info); scale: |s_a - s_b|; scale_info: info[4] relative to b's, over the poses where b's is positive."""
    ia, ib = np.asarray(a["info"], np.float64), np.asarray(b["info"], np.float64)
    pos = ib[:, 4] > 0
    return dict(ang=st.angle_and_rotation_distance(a, b), kp=float(np.linalg.norm(landmarks(c, a) - landmarks(c, b), axis=-1).max()),
                px=float(np.abs(ia[:, :2] - ib[:, :2]).max()),
                scale=float(np.abs(np.asarray(a["scale"], np.float64) - np.asarray(b["scale"], np.float64)).max()),
                scale_info=float((np.abs(ia[pos, 4] - ib[pos, 4]) / ib[pos, 4]).max()) if pos.any() else 0.0)


def float32_distance(c, want, max_iters=1):
    """The worst distance of the float32 restatements - one per solver of st.SOLVERS - from the float64 result `want`."""
    return st.worst([distance(c, restate(c, np.float32, max_iters, s), want) for s in st.SOLVERS])


def bounds_from(d32):
    """views_cases.bounds_from for ang, kp and px; scale and the scale information under the same rule: st.FLOAT32_FACTOR x the
    float32 restatements' distance, floors SCALE_TOL / INFO_RTOL."""
    return dict(vc.bounds_from(d32), scale=max(SCALE_TOL, st.FLOAT32_FACTOR * d32["scale"]),
                scale_info=max(INFO_RTOL, st.FLOAT32_FACTOR * d32["scale_info"]))


within = st.within


# ----------------------------------------------------------------------------- noisy windows and the 3-D chain
NOISY_SCALE = 1.1


@functools.lru_cache(maxsize=None)
def noisy_case(noise=1.0, seed=0, outliers=0):
    """The 74 golden hands in their two seeing views: exact windows of the label poses on the model scaled by NOISY_SCALE plus
    the Gaussian noise ic.noisy_windows draws (default_rng(seed).normal on the whole golden window array, `noise` px), and with
    `outliers` > 0 that many detections per hand (spread over its views by rc.contaminated's draw, seed 7) moved rc.OUTLIER_PX.
    init / init_scale = the float64 3-D chain on the same detections, rounded to float32: triangulation
    (tc.triangulate) -> sc.fit_scale, free and cold, on the points two views give (weights 1 / 0); `chain` holds its float64
    outputs.  Cached: leave it unchanged."""
    g = vc.golden()
    n = len(g["hand"])
    truth = vc.posed(g, sc.scaled_model(g["hm"], np.full(n, NOISY_SCALE)))
    exact = vc.exact_windows(g["table"], g["cam_rows"], truth)
    c = vc.select(g, g["seeing"], exact + np.random.default_rng(seed).normal(0.0, noise, g["window"].shape))
    c.update(hm=g["hm"], table=g["table"], mirror=g["hand"], t_scale=1.0, limits=None, truth=truth)
    if outliers:
        per_view = outliers // c["window"].shape[1]
        c = rc.contaminated(c, per_view, rc.OUTLIER_PX, 7)
    pts, tri, _res, _it = tc.triangulate(c["window"], c["cam_rows"], c["table"], c["weights"])
    status = tri[..., 3].astype(np.int64)
    used = ((status & (tc.REFUSED | tc.DEGENERATE)) == 0).astype(np.float64)
    target = np.where(used[..., None] > 0, pts, 0.0).astype(np.float32).astype(np.float64)
    ja, xf, s, info = sc.fit_scale(g["hm"], target, weights=used, mirror=g["hand"])
    c.update(init=(ja.astype(np.float32), xf.astype(np.float32)), init_scale=s.astype(np.float32), mode=FREE, true_scale=NOISY_SCALE,
             loss="squared", loss_scale=rc.SCALE_PX, chain=dict(ja=ja, xf=xf, scale=s, info=info, points=target, used=used))
    return c


def calibrate(c, dtype=np.float64, max_iters=32, solver="lu"):
    """The chain free pass -> sc.pool over all poses as one group -> fixed pass at the pooled scale, warm-started from the first:
    dict(free, stats [4], fixed)."""
    free = restate(c, dtype, max_iters, solver)
    stats = sc.pool(free["scale"], free["info"], len(free["scale"]))[0]
    again = dict(c, init=(free["ja"].astype(np.float32), free["xf"].astype(np.float32)), mode=FIXED,
                 init_scale=np.full(len(free["scale"]), np.float32(stats[0])))
    return dict(free=free, stats=stats, fixed=restate(again, dtype, max_iters, solver))
