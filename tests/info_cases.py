"""Shared by tests/test_info_host.py, tests/test_gpu_info.py and tools/bench_info.py: the numpy restatement of the two entries of
include/umetrack_hip_info.h, built on tests/triangulate_cases.py and tests/fit_cases.py.

`triangulate_info` is tc.triangulate plus the factor ut_triangulate_points_info hands out: the lower Cholesky factor of
H = sum_v w_v J_v^T J_v (tc._normal_equations) at the point tc.triangulate returns, by tc._chol, in float64.

`fit_info` is the loop of fc.fit - the same constants, accept / reject rule, Marquardt scaling, lambda schedule and stop rules -
on residuals and Jacobian rows whitened by a factor per landmark (csrc/fit_info.hip): `fit_info(..., dtype=np.float64)` is the
oracle, `dtype=np.float32` the same code in float32."""
import numpy as np

import fit_cases as fc
import triangulate_cases as tc

CONVERGED, AT_MAX_ITERS, REFUSED = fc.CONVERGED, fc.AT_MAX_ITERS, fc.REFUSED


# ----------------------------------------------------------------------------- the factor
def triangulate_info(window, cam_rows, table, weights=None, max_iters=16):
    """ut_triangulate_points_info in float64 numpy: tc.triangulate's (points, info, residual, iterations) and sqrt_info
    [n,P,6] float64 - (l00, l10, l11, l20, l21, l22), not yet rounded to float32; all 0 for refused and degenerate points and
    where the float32 sigma is +inf."""
    pts, info, residual, iters = tc.triangulate(window, cam_rows, table, weights, max_iters)
    window, table, cam_rows = np.asarray(window, np.float64), np.asarray(table, np.float64), np.asarray(cam_rows)
    n, v_max, n_pts = window.shape[:3]
    kind = tc.FISHEYE62 if table.shape[1] == 32 else tc.PINHOLE
    w_in = np.ones((n, v_max, n_pts)) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    big = n * n_pts
    win = window.transpose(0, 2, 1, 3).reshape(big, v_max, 2)
    w = w_in.transpose(0, 2, 1).reshape(big, v_max)
    rows = np.repeat(cam_rows[:, None, :], n_pts, 1).reshape(big, v_max)
    tab = table[np.maximum(rows, 0)]
    with np.errstate(all="ignore"):                      # step 1 of tc.triangulate: the used views
        ok = (rows >= 0) & np.isfinite(w) & (w > 0) & np.isfinite(win).all(-1)
        safe_win = np.where(ok[..., None], win, 0.0)
        used = ok & np.isfinite(tc.unproject(tab, safe_win, kind)[1]).all(-1)
    _cost, h, _g, _good, _dist = tc._normal_equations(tab, safe_win, w, used, pts.reshape(big, 3), kind)
    l, factored = tc._chol(h, np.zeros(big))
    status = info.reshape(big, 4)[:, 3].astype(int)
    known = ((status & (tc.REFUSED | tc.DEGENERATE)) == 0) & factored & np.isfinite(info.reshape(big, 4)[:, 1])
    with np.errstate(all="ignore"):
        sqrt_info = np.where(known[:, None], np.stack(l, -1), 0.0)
    return pts, info, residual, iters, sqrt_info.reshape(n, n_pts, 6)


def matrix(sqrt_info):
    """[...,6] -> the lower triangular L [...,3,3]."""
    f = np.asarray(sqrt_info)
    m = np.zeros(f.shape[:-1] + (3, 3), f.dtype)
    m[..., 0, 0], m[..., 1, 0], m[..., 1, 1], m[..., 2, 0], m[..., 2, 1], m[..., 2, 2] = (f[..., k] for k in range(6))
    return m


def isotropic(weights):
    """The factors sqrt(w) I of scalar weights [...]: ut_fit_pose's cost."""
    s = np.sqrt(np.asarray(weights))
    out = np.zeros(s.shape + (6,), s.dtype)
    out[..., 0], out[..., 2], out[..., 5] = s, s, s
    return out


def whiten(f, r):
    """L^T r for factors f [B,21,6] and r [B,21,3,...]: (l00 r0 + l10 r1 + l20 r2, l11 r1 + l21 r2, l22 r2)."""
    l = [f[..., k].reshape(f.shape[:2] + (1,) * (r.ndim - 3)) for k in range(6)]
    r0, r1, r2 = r[:, :, 0], r[:, :, 1], r[:, :, 2]
    return np.stack([l[0] * r0 + l[1] * r1 + l[3] * r2, l[2] * r1 + l[4] * r2, l[5] * r2], 2)


# ----------------------------------------------------------------------------- the fit
class _Whitened(fc.Problem):
    """fc.Problem with the residuals and the Jacobian rows of every landmark whitened by its factor f [B,21,6]; w is the
    factor's squared Frobenius norm, n_used [B] the number of used landmarks."""

    def __init__(self, hm, dtype, f, w, used, y, refused, n_used):
        super().__init__(hm, dtype, w, used, y, refused)
        self.f, self.n_used = f, n_used

    def pivot(self, ang, m):
        centroid, extent, _wsum = super().pivot(ang, m)
        return centroid, extent, (3 * self.n_used).astype(self.dt)

    def _residuals(self, idx, ang, m):
        r = np.where(self.used[idx][..., None], fc.forward(fc._take(self.hm, idx), ang, m, self.dt) - self.y[idx], self.dt(0))
        return r, whiten(self.f[idx], r)

    def system(self, idx, ang, m, centroid):
        k = len(idx)
        jac = fc.jacobian(fc._take(self.hm, idx), ang, m, centroid, self.dt).reshape(k, 21, 3, 26)
        jac = whiten(self.f[idx], np.where(self.used[idx][..., None, None], jac, self.dt(0))).reshape(k, 63, 26)
        return jac, self._residuals(idx, ang, m)[1].reshape(k, 63)

    def cost(self, idx, ang, m, extra=None):
        r, u = self._residuals(idx, ang, m)
        with np.errstate(invalid="ignore", over="ignore"):
            return (u * u).sum((1, 2)), np.sqrt((r * r).sum(-1).max(1))


def fit_info(hm, targets, sqrt_info, limits=None, init=None, mirror=None, t_scale=1.0, max_iters=32, dtype=np.float64,
             trace=None):
    """ut_fit_pose_info: fc.fit with the cost sum_l |L_l^T (landmark_l - target_l)|^2.  sqrt_info [B,21,6]; every other argument
    (trace included) and the outputs as for fc.fit, with info [B,4]: sqrt(cost / (3 used landmarks)), the largest Euclidean
    residual of a used landmark, iterations, status.  A landmark is used when any entry of its factor is non-zero; its scalar weight (centroid,
    extent, the cold start's Kabsch fit) is the factor's squared Frobenius norm.  Refused: a factor entry that is not finite,
    a non-finite target of a used landmark, fewer than 3 used landmarks."""
    dt = dtype
    f = np.asarray(sqrt_info).astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        bad_f = ~np.isfinite(f).all((1, 2)) | ~np.isfinite((f * f).sum(-1)).all(1)
        used = (f != 0).any(-1) & ~bad_f[:, None]
        refused = bad_f | (used.sum(1) < 3) | (~np.isfinite(np.asarray(targets)) & used[..., None]).any((1, 2))
    used &= ~refused[:, None]
    f = np.where(used[..., None], f, dt(0))
    w = np.where(refused[:, None], dt(1), (f * f).sum(-1))
    n_used = np.where(refused, 21, used.sum(1))
    y = np.where(used[..., None], np.asarray(targets), 0).astype(dt)
    return fc.lm(_Whitened(hm, dt, f, w, used, y, refused, n_used), limits, init, mirror, t_scale, max_iters, trace=trace)


# ----------------------------------------------------------------------------- the golden chain
def golden_hands():
    """tc.golden_case() with the skeleton and mirror flags of its 74 hands (recording_00's model; `hand` of
    tests/golden/projection_rec00.npz)."""
    import os

    import mesh_cases as mc
    from absolutetrack_amd import pipeline
    g = tc.golden_case()
    z = np.load(os.path.join(tc.GOLDEN, "projection_rec00.npz"))
    g["hm"] = mc.skeleton(np.load(pipeline._DATA), "hm.")
    g["hand"] = z["hand"].astype(np.int64)
    return g


def noisy_windows(g, noise, seed):
    """The golden windows plus Gaussian noise of `noise` px: default_rng(seed).normal on the whole window array."""
    return g["window"] + np.random.default_rng(seed).normal(0.0, noise, g["window"].shape)


def chain(g, window, dtype=np.float64, max_iters=32):
    """Triangulation with factor -> isotropic fit on the used landmarks (weights 1 / 0, cold) -> information fit started from
    it.  Returns dict(points, sqrt_info (rounded to float32, as the kernel hands it out), iso = fc.fit's outputs, info =
    fit_info's)."""
    pts, tri, _res, _it, factor = triangulate_info(window, g["cam_rows"], g["table"], g["weights"])
    factor = factor.astype(np.float32).astype(np.float64)
    target = pts.astype(np.float32).astype(np.float64)
    used = (factor != 0).any(-1).astype(np.float64)
    iso = fc.fit(g["hm"], target, weights=used, mirror=g["hand"], max_iters=max_iters, dtype=dtype)
    inf = fit_info(g["hm"], target, factor, init=(iso[0], iso[1]), mirror=g["hand"], max_iters=max_iters, dtype=dtype)
    return dict(points=target, tri=tri, sqrt_info=factor, iso=iso, info=inf)


def landmarks_of(g, ja, xf, dtype=np.float64):
    return fc.forward(g["hm"], np.asarray(ja, dtype)[:, :20], fc.effective_wrist(np.asarray(xf, dtype), g["hand"], 1.0, dtype), dtype)
