"""Shared by tests/test_uncertainty_host.py, tests/test_gpu_uncertainty.py and tools/bench_uncertainty.py: the numpy restatement
of ut_pose_information_views (include/umetrack_hip_uncertainty.h, csrc/pose_info_views.hip) and the cases its tests share.

`information` is built on views_cases and robust_cases and restates nothing they state: the pivot is vc.pivot, the 63 reduced
rows are vc.reduced_system on rc.RobustViews (which carries psi), the landmarks' world Jacobian G is fc.jacobian.  Its own part
is what the kernel adds: H = J^T J (+ 1 / sigma^2 on the angles' diagonal), the scaling to unit diagonal, the pivot rule
(MIN_PIVOT, a pivot being the diagonal of the Schur complement), param_sigma = sqrt(diag H^-1) and Sigma_l = G_l H^-1 G_l^T.
`information(..., dtype=np.float64)` is the oracle, `dtype=np.float32` the same code in float32, with the inverse through
numpy's LU ("lu") or through the Cholesky factor and forward substitutions, the kernel's algorithm ("cholesky") - st.RUNS.  The
status is the Cholesky pivot rule's with either inverse."""
import functools

import numpy as np

import fit_cases as fc
import robust_cases as rc
import step_cases as st
import views_cases as vc

OK, SINGULAR, REFUSED = 1, 2, 4                          # UT_COV_*
MIN_PIVOT = 2.0 ** -16                                   # UT_COV_MIN_PIVOT
INFO_FLOOR = 63 * 2.0 ** -24                             # the rounding of one 63-term float32 dot product, relative
PIVOT_UNIT = 2.0 ** -23                                  # x the landmarks' extent: one float32 ulp of a coordinate


def tril(h):
    """[n,26,26] -> the packed lower triangle [n,351], row-major, as the entry writes it."""
    i, j = np.tril_indices(26)
    return h[:, i, j]


def untril(packed):
    """[n,351] -> symmetric [n,26,26]."""
    packed = np.asarray(packed)
    i, j = np.tril_indices(26)
    h = np.zeros(packed.shape[:-1] + (26, 26), packed.dtype)
    h[..., i, j] = packed
    h[..., j, i] = packed
    return h


def uncov(packed):
    """(xx, yx, yy, zx, zy, zz) [...,6] -> symmetric [...,3,3]."""
    packed = np.asarray(packed)
    out = np.zeros(packed.shape[:-1] + (3, 3), packed.dtype)
    for n, (a, b) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        out[..., a, b] = out[..., b, a] = packed[..., n]
    return out


def scaled_factor(h):
    """The Cholesky factor of D^-1/2 H D^-1/2 (unit diagonal), right-looking in the dtype of h as the kernel runs it:
    (L [n,26,26], sqrt(D) [n,26], smallest pivot [n], regular [n]).  A diagonal entry of H that is not positive gives pivot 0; the
    factorisation of a pose stops at its first pivot <= MIN_PIVOT, which still counts for the smallest."""
    dt = h.dtype.type
    n = h.shape[0]
    d = np.einsum("nii->ni", h)
    has = (d > 0) & np.isfinite(d)
    sd = np.where(has, np.sqrt(np.where(has, d, 1)), 0).astype(dt)
    s = np.where(has, 1 / np.where(has, sd, 1), 0).astype(dt)
    a = (h * s[:, :, None] * s[:, None, :]).astype(dt)
    k = np.arange(26)
    a[:, k, k] = has.astype(dt)
    low = np.zeros_like(a)
    alive, least = np.ones(n, bool), np.ones(n, dt)
    with np.errstate(all="ignore"):
        for j in range(26):
            piv = a[:, j, j]
            good = (piv > MIN_PIVOT) & np.isfinite(piv)
            seen = np.where(good, piv, np.where(piv > 0, piv, 0)).astype(dt)
            least = np.where(alive, np.minimum(least, seen), least)
            alive &= good
            root = np.sqrt(np.where(alive, piv, 1)).astype(dt)
            low[:, j:, j] = a[:, j:, j] / root[:, None]
            a[:, j + 1:, j + 1:] -= low[:, j + 1:, j, None] * low[:, None, j + 1:, j]
    return low, sd, least, alive


def forward_substitution(low, rhs):
    """low y = rhs, [n,26,26] and [n,26,k], in their dtype."""
    y = np.zeros_like(rhs)
    for i in range(low.shape[-1]):
        y[:, i] = (rhs[:, i] - np.einsum("nj,njk->nk", low[:, i, :i], y[:, :i])) / low[:, i, i, None]
    return y


def information(c, dtype=np.float64, inverse="lu", drop=()):
    """ut_pose_information_views on a case (below): dict(pose_info [n,26,26], pivot [n,3], param_sigma [n,26], landmark_cov
    [n,21,3,3], info [n,4]: rms of the cost at the pose, largest landmark sigma, smallest scaled pivot, status) in dtype.
    drop: what a deliberately wrong restatement leaves out - "psi", "prior" or "pivot" (H's rotation then turns about the origin
    while the landmarks' Jacobian G still turns about the centroid)."""
    n = len(c["ja"])
    idx = np.arange(n)
    loss = "squared" if "psi" in drop else c["loss"]
    vw = rc.RobustViews(c["window"], c["cam_rows"], c["table"], c["weights"], dtype, loss, c["loss_scale"])
    ang = np.asarray(c["ja"])[:, :20].astype(dtype)
    m = fc.effective_wrist(c["xf"], c["mirror"], c["t_scale"], dtype)
    hm = c["hm"]
    with np.errstate(all="ignore"):
        p = fc.forward(hm, ang, m, dtype)
        centroid, _extent, wsum = vc.pivot(vw, p, dtype)
        about = np.zeros_like(centroid) if "pivot" in drop else centroid
        cost = rc.RobustViews(c["window"], c["cam_rows"], c["table"], c["weights"], dtype, c["loss"], c["loss_scale"]).cost(p, idx, dtype)[0]
        sigma = None if c.get("angle_sigma") is None or "prior" in drop else np.broadcast_to(
            np.asarray(c["angle_sigma"], np.float32).reshape(-1, 20), (n, 20)).astype(dtype)
        refused = vw.refused | ~np.isfinite(cost)
        if sigma is not None:
            s32 = sigma.astype(np.float32)
            refused = refused | ~(np.isfinite(s32) & (s32 > 0) & np.isfinite(np.float32(1) / (s32 * s32))).all(1)
        jac, _r = vc.reduced_system(vw, hm, ang, m, about, idx, dtype)
        h = (jac.transpose(0, 2, 1) @ jac).astype(dtype)
        if sigma is not None:
            k = np.arange(20)
            h[:, k, k] += (1 / (sigma * sigma)).astype(dtype)
        h = np.where(refused[:, None, None], dtype(0), h)
        g = fc.jacobian(hm, ang, m, centroid, dtype)                          # [n,63,26]
        low, sd, least, regular = scaled_factor(h)
        regular &= ~refused
        solve = np.where(regular[:, None, None], low * sd[:, :, None], np.eye(26, dtype=dtype))      # the factor of H itself
        if inverse == "cholesky":
            y = forward_substitution(solve, np.concatenate([g.transpose(0, 2, 1), np.broadcast_to(np.eye(26, dtype=dtype), (n, 26, 26))], 2))
            yg, ye = y[:, :, :63].reshape(n, 26, 21, 3), y[:, :, 63:]
            cov = np.einsum("nkla,nklb->nlab", yg, yg)
            var = (ye * ye).sum(1)
        else:
            assert inverse == "lu", inverse
            sc = np.where(sd > 0, 1 / np.where(sd > 0, sd, 1), 0).astype(dtype)
            unit = np.where(regular[:, None, None], h * sc[:, :, None] * sc[:, None, :], np.eye(26, dtype=dtype)).astype(dtype)
            inv = np.linalg.inv(unit) * sc[:, :, None] * sc[:, None, :]
            gl = g.reshape(n, 21, 3, 26)
            cov = np.einsum("nlak,nkj,nlbj->nlab", gl, inv, gl)
            var = np.einsum("nii->ni", inv)
        sig = np.sqrt(var)
        unknown = np.where(np.eye(3, dtype=bool), dtype(np.inf), dtype(0))
        cov = np.where(regular[:, None, None, None], cov, unknown)
        sig = np.where(regular[:, None], sig, dtype(np.inf))
        worst = np.sqrt(np.einsum("nlaa->nl", cov).max(1))
        rms = np.sqrt(cost / wsum)
    status = np.where(refused, REFUSED, np.where(regular, OK, SINGULAR))
    info = np.stack([rms, worst, least, status.astype(dtype)], 1)
    out = dict(pose_info=h, pivot=centroid, param_sigma=sig, landmark_cov=cov, info=info)
    for k, v in out.items():
        zero = refused.reshape((n,) + (1,) * (v.ndim - 1))
        out[k] = np.where(zero, dtype(0), v).astype(dtype)
    out["info"][:, 3] = status
    return out


# ----------------------------------------------------------------------------- distances and bounds
QUANTITIES = ("pose_info", "landmark_cov", "param_sigma", "pivot", "rms", "least")


def extent(c):
    """The landmarks' extent per pose: the largest |coordinate| of the float64 landmarks, what a float32 coordinate rounds at."""
    m = fc.effective_wrist(np.asarray(c["xf"], np.float64), c["mirror"], c["t_scale"], np.float64)
    return np.abs(fc.forward(c["hm"], np.asarray(c["ja"], np.float64)[:, :20], m, np.float64)).max((1, 2))


def distance(c, got, want):
    """How far a result lies from the float64 one `want`, over the poses float64 calls regular (pose_info and pivot: over those it
    does not refuse).  pose_info: max |dH_ij| / sqrt(H_ii H_jj), an entry with a zero diagonal partner must be equal; landmark_cov:
    max_l |dSigma_l|_F / tr Sigma_l; param_sigma: relative; pivot: absolute, in units of the landmarks' extent x 2^-23; rms and
    least: info[0] in px and info[2], the smallest pivot of the unit-diagonal matrix, absolute."""
    status = want["info"][:, 3].astype(np.int64)
    wrote, reg = status != REFUSED, status == OK
    hw, hg = np.asarray(want["pose_info"], np.float64), np.asarray(got["pose_info"], np.float64)
    d = np.einsum("nii->ni", hw)
    den = np.sqrt(d[:, :, None] * d[:, None, :])
    with np.errstate(all="ignore"):
        rel = np.where(den > 0, np.abs(hg - hw) / np.where(den > 0, den, 1), np.where(hg == hw, 0.0, np.inf))
        out = dict(pose_info=float(rel[wrote].max()) if wrote.any() else 0.0)
        cw, cg = np.asarray(want["landmark_cov"], np.float64)[reg], np.asarray(got["landmark_cov"], np.float64)[reg]
        out["landmark_cov"] = float((np.sqrt(((cg - cw) ** 2).sum((2, 3))) / np.einsum("nlaa->nl", cw)).max()) if reg.any() else 0.0
        sw, sg = np.asarray(want["param_sigma"], np.float64)[reg], np.asarray(got["param_sigma"], np.float64)[reg]
        out["param_sigma"] = float((np.abs(sg - sw) / sw).max()) if reg.any() else 0.0
        dp = np.abs(np.asarray(got["pivot"], np.float64) - np.asarray(want["pivot"], np.float64)).max(1) / (extent(c) * PIVOT_UNIT)
        out["pivot"] = float(dp[wrote].max()) if wrote.any() else 0.0
        di = np.abs(np.asarray(got["info"], np.float64) - np.asarray(want["info"], np.float64))
        out["rms"], out["least"] = float(di[:, 0].max()), float(di[:, 2].max())
    return {k: (v if np.isfinite(v) else np.inf) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """information(case(name)) in float64.  Cached: leave it unchanged."""
    return information(case(name))


@functools.lru_cache(maxsize=None)
def float32_distance(name):
    """The worst distance of the two float32 restatements (st.SOLVERS' inverses) from float64 on case(name)."""
    c, want = case(name), oracle(name)
    return st.worst([distance(c, information(c, np.float32, s), want) for s in st.SOLVERS])


def bounds_from(d32):
    """DESIGN's rule for one step against float64: st.FLOAT32_FACTOR x the float32 restatements' own distance.  pose_info never
    below the factor x INFO_FLOOR, the pivot never below the factor x one unit (one float32 ulp of a coordinate), the rms never
    below what rounding the float64 figure to float32 costs at 300 px (views_cases.bounds_from), the smallest pivot never below
    the factor x 26 x 2^-24 (one row of the unit-diagonal factorisation: 26 roundings of terms <= 1)."""
    f = st.FLOAT32_FACTOR
    return dict(pose_info=f * max(INFO_FLOOR, d32["pose_info"]), landmark_cov=f * d32["landmark_cov"], param_sigma=f * d32["param_sigma"],
                pivot=f * max(1.0, d32["pivot"]), rms=max(300.0 * 2.0 ** -23, f * d32["rms"]), least=f * max(26 * 2.0 ** -24, d32["least"]))


within = st.within


# ----------------------------------------------------------------------------- cases
REGULAR = ("two_views", "best_view", "ragged", "spread", "pinhole", "metres", "mixed")
ROBUST = ("outliers_huber", "outliers_geman_mcclure")
CASES = REGULAR + ROBUST + ("free_finger", "free_finger_prior")
OUTLIER_SCALE_PX = 2.0
FREE_FINGER = 1                                          # the index finger: columns 4 .. 7


def label_pose(c):
    """The label poses of the golden hands as float32 records of the case: the translation in the case's units."""
    g = vc.golden()
    xf = np.array(g["xf"], np.float64, copy=True)
    xf[:, :3, 3] /= c["t_scale"]
    return np.asarray(g["ja"], np.float32).copy(), xf.astype(np.float32)


def angle_sigma_from_limits(limits):
    """(hi - lo) / sqrt(12), float32: what hand.angle_sigma_from_limits returns."""
    limits = np.asarray(limits, np.float32)
    return ((limits[..., 1] - limits[..., 0]) / np.float32(np.sqrt(12.0))).astype(np.float32)


def free_columns(c):
    """[n,26] bool: the parameters no used landmark of the pose depends on, from the float64 world Jacobian."""
    vw = vc.Views(c["window"], c["cam_rows"], c["table"], c["weights"], np.float64)
    m = fc.effective_wrist(c["xf"], c["mirror"], c["t_scale"], np.float64)
    ang = np.asarray(c["ja"], np.float64)[:, :20]
    g = fc.jacobian(c["hm"], ang, m, np.zeros((len(ang), 3)), np.float64).reshape(len(ang), 21, 3, 26)
    return ~((g != 0).any(2) & vw.used.any(1)[:, :, None]).any(1)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case `name` on the 74 golden hands at their label poses: views_cases.case's inputs as copies, and ja, xf (the pose,
    float32), loss, loss_scale, angle_sigma.  REGULAR: vc.case(name) under the squared loss.  ROBUST: two_views with 2 detections of
    every view displaced by 40 px (rc.contaminated, seed 7) under the loss at 2 px.  free_finger: two_views with every landmark
    that moves with the index finger at weight 0 in all views - its four angles are free: the singular case; free_finger_prior:
    the same with angle_sigma from the stock joint limits.  Cached: leave it unchanged."""
    base = vc.case(name if name in REGULAR else "two_views")
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items() if k != "init"}
    c.update(loss="squared", loss_scale=rc.SCALE_PX, angle_sigma=None)
    c["ja"], c["xf"] = label_pose(c)
    if name in ROBUST:
        c = rc.contaminated(c, rc.OUTLIERS, rc.OUTLIER_PX, 7)
        c.update(loss=name[len("outliers_"):], loss_scale=OUTLIER_SCALE_PX)
    if name.startswith("free_finger"):
        m = fc.effective_wrist(c["xf"], c["mirror"], c["t_scale"], np.float64)
        g = fc.jacobian(c["hm"], np.asarray(c["ja"], np.float64)[:, :20], m, np.zeros((len(m), 3)), np.float64).reshape(len(m), 21, 3, 26)
        moves = (g[..., 4 * FREE_FINGER:4 * FREE_FINGER + 4] != 0).any((2, 3))              # [n,21]
        c["weights"] = np.where(moves[:, None, :], np.float32(0), c["weights"]).astype(np.float32)
        if name == "free_finger_prior":
            c["angle_sigma"] = angle_sigma_from_limits(st.joint_limits())
    else:
        assert name in REGULAR + ROBUST, name
    return c


def subset(c, sel):
    """Poses sel of a case."""
    sel = np.asarray(sel)
    out = dict(c, hm=fc._take(c["hm"], sel))
    for k in ("window", "cam_rows", "weights", "mirror", "truth", "ja", "xf", "displaced"):
        if k in c:
            out[k] = c[k][sel]
    if c.get("angle_sigma") is not None and np.asarray(c["angle_sigma"]).ndim == 2 and len(c["angle_sigma"]) == len(c["ja"]):
        out["angle_sigma"] = c["angle_sigma"][sel]
    return out


def take(res, sel):
    return {k: np.asarray(v)[np.asarray(sel)] for k, v in res.items()}
