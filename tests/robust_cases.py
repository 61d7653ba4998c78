"""Shared by tests/test_robust_host.py, tests/test_gpu_robust.py and tools/bench_robust.py: the numpy restatement of
ut_fit_pose_views_robust (include/umetrack_hip_robust.h, csrc/fit_views_robust.hip, csrc/ut_fit_views_dev.h) and the cases its
tests share.

The restatement is views_cases' with one method replaced: `RobustViews.blocks` forms the per-landmark cost with c^2 rho(d^2 / c^2)
where views_cases.Views has d^2, and M and b with w_v psi_v where it has w_v - psi in float64 from the residual, the views in
ascending order, as the kernel does.  Everything else - the semidefinite 3 x 3 Cholesky, the reduction to 63 rows, the pivot at
the start's centroid, and the loop fc.lm with its accept / reject rule, lambda schedule and stop rules - is views_cases' and
fit_cases' code, run unchanged on the robust cost.  With the loss "squared" psi is the constant 1.0 and the restatement is
views_cases.fit_views bit for bit (tests/test_robust_host.py).

Why full fits are judged only on selected hands: on contaminated data the cost has valleys along depth and several basins, so
two correct solvers can end 0.6 mm apart and iteration counts scatter up to max_iters.  One solver step is well conditioned for
every loss; the sharp GPU checks are one-step checks."""
import functools

import numpy as np

import fit_cases as fc
import step_cases as st
import views_cases as vc

LOSSES = ("squared", "huber", "geman_mcclure")          # UT_LOSS_SQUARED, UT_LOSS_HUBER, UT_LOSS_GEMAN_MCCLURE
ROBUST = LOSSES[1:]
INLIER_FLOOR = 2.0 ** -24                                # one float32 rounding of a value <= 1


# ----------------------------------------------------------------------------- the loss
def scale_squared(loss_scale):
    """(c^2, 1 / c^2) in float64 of the float32 scale the entry receives, as the kernel forms them."""
    c = float(np.float32(loss_scale))
    return c * c, 1.0 / (c * c)


def psi(loss, d2, loss_scale):
    """rho'(d2 / c^2), float64: the weight of an observation at squared reprojection distance d2."""
    d2 = np.asarray(d2, np.float64)
    if loss == "squared":
        return np.ones_like(d2)
    s = d2 * scale_squared(loss_scale)[1]
    with np.errstate(all="ignore"):
        if loss == "huber":
            return np.minimum(1.0, 1.0 / np.sqrt(s))
        assert loss == "geman_mcclure", loss
        return 1.0 / ((1.0 + s) * (1.0 + s))


def rho(loss, d2, loss_scale):
    """c^2 rho(d2 / c^2), float64: what an observation at squared reprojection distance d2 costs at weight 1."""
    d2 = np.asarray(d2, np.float64)
    if loss == "squared":
        return d2
    c2, inv_c2 = scale_squared(loss_scale)
    s = d2 * inv_c2
    with np.errstate(all="ignore"):
        if loss == "huber":
            return np.where(s <= 1.0, d2, 2.0 * d2 / np.sqrt(s) - c2)             # c^2 (2 sqrt(s) - 1)
        assert loss == "geman_mcclure", loss
        return d2 / (1.0 + s)


# ----------------------------------------------------------------------------- the observations
class RobustViews(vc.Views):
    """vc.Views whose blocks carry the loss: cost = sum_v w_v c^2 rho(d_v^2 / c^2), M = sum_v w_v psi_v J_v^T J_v and
    b = sum_v w_v psi_v J_v^T r_v, float64, views ascending.  `good`, the squared distances, the residuals and the Jacobians are
    views_cases', so `cost()`'s largest distance stays the raw one."""

    def __init__(self, window, cam_rows, table, weights, dtype, loss, loss_scale):
        super().__init__(window, cam_rows, table, weights, dtype)
        if loss not in LOSSES or (loss != "squared" and not (np.isfinite(loss_scale) and loss_scale > 0)):
            raise ValueError("bad loss or loss_scale")
        self.loss, self.loss_scale = loss, loss_scale

    def blocks(self, p, idx):
        _cost, _m, _g, good, sq_all, res, jacs = super().blocks(p, idx)
        k = len(idx)
        cost = np.zeros((k, 21))
        m = [np.zeros((k, 21)) for _ in range(6)]
        g = [np.zeros((k, 21)) for _ in range(3)]
        with np.errstate(all="ignore"):
            for v in range(self.v_max):
                r, jac = res[v], jacs[v]
                cost = cost + self.w[idx, v] * rho(self.loss, sq_all[:, v], self.loss_scale)
                wv = self.w[idx, v] * psi(self.loss, sq_all[:, v], self.loss_scale)
                n = 0
                for a in range(3):
                    for c in range(a + 1):
                        m[n] = m[n] + wv * (jac[..., 0, a] * jac[..., 0, c] + jac[..., 1, a] * jac[..., 1, c])
                        n += 1
                    g[a] = g[a] + wv * (jac[..., 0, a] * r[..., 0] + jac[..., 1, a] * r[..., 1])
            good = good & np.isfinite(cost)
        return cost, m, g, good, sq_all, res, jacs

    def inliers(self, p, idx):
        """psi of every used observation of poses idx at landmarks p, float64 [k,V,21]; 0 elsewhere."""
        sq = self.blocks(p, idx)[4]
        return np.where(self.used[idx], psi(self.loss, sq, self.loss_scale), 0.0)


class _Robust(vc._Reprojection):
    """vc._Reprojection on RobustViews; after the fit also `inlier` [B,V,21], float64: psi at the returned pose, 0 where unused or
    refused."""

    def report(self, refused, ang, m, centroid, status):
        columns = super().report(refused, ang, m, centroid, status)
        with np.errstate(all="ignore"):
            psi_end = self.vw.inliers(fc.forward(self.hm, ang, m, self.dt), np.arange(len(refused)))
        self.inlier = np.where(refused[:, None, None], 0.0, psi_end)
        return columns


def fit_views_robust(hm, window, cam_rows, table, weights=None, init=None, mirror=None, limits=None, t_scale=1.0, max_iters=32,
                     loss="squared", loss_scale=3.0, dtype=np.float64, solver="lu", trace=None):
    """ut_fit_pose_views_robust: views_cases.fit_views' tuple - info[0] = sqrt(robust cost / sum of the used weights), info[1] and
    residual raw distances - and inlier [B,V,21] float64."""
    if init is None:
        raise ValueError("init is required: there is no cold start")
    prob = _Robust(hm, dtype, RobustViews(window, cam_rows, table, weights, dtype, loss, loss_scale))
    with st.solver(solver):
        return fc.lm(prob, limits, init, mirror, t_scale, max_iters, trace=trace) + (prob.residual, prob.inlier)


def restate(c, dtype=np.float64, max_iters=1, solver="lu", trace=None):
    """fit_views_robust on a case (a views_cases case with `loss` and `loss_scale`): dict(ja, xf, info, residual, inlier)."""
    out = fit_views_robust(c["hm"], c["window"], c["cam_rows"], c["table"], c["weights"], c["init"], c["mirror"], c["limits"],
                           c["t_scale"], max_iters, c["loss"], c["loss_scale"], dtype, solver, trace)
    return dict(zip(("ja", "xf", "info", "residual", "inlier"), out))


def views_of(c, dtype=np.float64):
    return RobustViews(c["window"], c["cam_rows"], c["table"], c["weights"], dtype, c["loss"], c["loss_scale"])


def robust_cost(c, res):
    """The robust cost [n] of a result's pose, float64 throughout: float64 forward function, float64 sums."""
    return views_of(c).cost(vc.landmarks(c, res), np.arange(len(c["mirror"])), np.float64)[0]


def psi_at(c, res):
    """The float64 psi [n,V,21] at a result's returned pose: float64 forward function, float64 projection; 0 where unused or
    refused."""
    refused = (np.asarray(res["info"])[:, 3].astype(np.int64) & vc.REFUSED) != 0
    with np.errstate(all="ignore"):
        at = views_of(c).inliers(vc.landmarks(c, res), np.arange(len(refused)))
    return np.where(refused[:, None, None], 0.0, at)


def distance(c, a, b):
    """views_cases.distance of a from b and `inlier`: how far a's inlier output lies from the float64 psi at a's own returned
    pose.  How far two poses lie apart is what ang and kp measure; `inlier` measures the output itself."""
    return dict(vc.distance(c, a, b), inlier=float(np.abs(np.asarray(a["inlier"], np.float64) - psi_at(c, a)).max()))


def float32_distance(c, want, max_iters=1):
    """The worst distance of the float32 restatements - one per solver of st.SOLVERS - from the float64 result `want`."""
    return st.worst([distance(c, restate(c, np.float32, max_iters, s), want) for s in st.SOLVERS])


def bounds_from(d32):
    """views_cases.bounds_from, and for `inlier` st.FLOAT32_FACTOR x the float32 restatements' distance from the float64 psi at
    their returned poses, never below one float32 rounding of a value <= 1."""
    return dict(vc.bounds_from(d32), inlier=max(INLIER_FLOOR, st.FLOAT32_FACTOR * d32["inlier"]))


# ----------------------------------------------------------------------------- cases
def with_loss(c, loss, loss_scale=3.0):
    return dict(c, loss=loss, loss_scale=loss_scale)


def contaminated(c, k, shift_px, seed):
    """The case with k used detections per view and pose displaced by shift_px in random directions; weights, and with them the
    mask of used observations, are kept.  `displaced` [n,V,21] marks them."""
    rng = np.random.default_rng(seed)
    used = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64).used
    win, displaced = c["window"].copy(), np.zeros(used.shape, bool)
    for i in range(used.shape[0]):
        for v in range(used.shape[1]):
            cand = np.nonzero(used[i, v])[0]
            if len(cand) < k:
                continue
            hit = rng.choice(cand, k, replace=False)
            phi = rng.uniform(0.0, 2.0 * np.pi, k)
            win[i, v, hit] += shift_px * np.stack([np.cos(phi), np.sin(phi)], -1)
            displaced[i, v, hit] = True
    return dict(c, window=win, displaced=displaced)


def tracking_starts(g, seed=53):
    """A tracking start: the label poses +-0.05 rad on the angles and the wrist's rotation vector, +-5 mm; float32."""
    return st.perturbed(g["ja"], g["xf"], seed, 0.05, 0.05, 5.0)


STEP_CASES = ("two_views", "best_view", "ragged", "spread", "pinhole", "metres", "mixed")
OUTLIERS, OUTLIER_PX, SCALE_PX = 2, 40.0, 3.0


@functools.lru_cache(maxsize=None)
def step_case(name, loss, loss_scale=SCALE_PX, dirty=False):
    """views_cases.case(name) - exact windows, starts +-0.2 rad / +-15 mm - under a loss; dirty: OUTLIERS detections per view
    displaced by OUTLIER_PX (seed 7).  Cached: leave it unchanged."""
    c = vc.case(name)
    return with_loss(contaminated(c, OUTLIERS, OUTLIER_PX, 7) if dirty else c, loss, loss_scale)


@functools.lru_cache(maxsize=None)
def tracked_case(views, loss, k=OUTLIERS, loss_scale=SCALE_PX):
    """The 74 golden hands in their two seeing views ('two') or the best view alone ('one'): exact windows of the label poses
    with k detections per view displaced by OUTLIER_PX (seed 7), tracking starts.  Cached: leave it unchanged."""
    base = vc.case("two_views" if views == "two" else "best_view")
    ja0, xf0 = tracking_starts(vc.golden())
    return with_loss(contaminated(dict(base, init=(ja0, xf0)), k, OUTLIER_PX, 7), loss, loss_scale)


SELECT_ITERS, SELECT_MM = 24, 0.1


@functools.lru_cache(maxsize=None)
def selected():
    """The hands of tracked_case('two', 'geman_mcclure') on which full fits can be judged: every restatement of st.RUNS converges
    within SELECT_ITERS iterations (max_iters 32), float64 ends within SELECT_MM of the truth and both float32 runs within
    vc.BASIN_MM.  Returns (indices, the runs' results, their landmark errors [3,74] in mm).  Cached: leave it unchanged."""
    c = tracked_case("two", "geman_mcclure")
    ok = np.ones(len(c["mirror"]), bool)
    runs, errs = [], []
    for dt, how in st.RUNS:
        r = restate(c, dt, 32, how)
        err = np.linalg.norm(vc.landmarks(c, r) - c["truth"], axis=-1).max(1)
        ok &= (r["info"][:, 3] == vc.CONVERGED) & (r["info"][:, 2] <= SELECT_ITERS) & (err <= (SELECT_MM if dt is np.float64 else vc.BASIN_MM))
        runs.append(r)
        errs.append(err)
    return np.nonzero(ok)[0], runs, np.stack(errs)


def subset(c, sel):
    out = vc.subset(c, sel)
    if "displaced" in c:
        out["displaced"] = c["displaced"][np.asarray(sel)]
    return out
