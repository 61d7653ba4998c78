"""Shared by tests/test_views_host.py, tests/test_gpu_views.py and tools/bench_views.py: the numpy restatement of
ut_fit_pose_views (include/umetrack_hip_views.h, csrc/fit_views.hip) and the cases its tests share.

`fit_views` is the loop of fc.fit - the same constants, accept / reject rule, Marquardt scaling, lambda schedule and stop rules -
on the reprojection cost sum_v sum_l w_vl |project_v(landmark_l) - window_vl|^2, built on fit_cases (forward, jacobian,
apply_step, solve, the constants) and triangulate_cases.project(..., jacobian=True).  It takes the kernel's decisions: the same
refusals, the views in ascending order, per landmark M = sum_v w_v J_v^T J_v and b = sum_v w_v J_v^T r_v in float64 on the
landmark of the working precision, the semidefinite 3 x 3 Cholesky M = L L^T with tc.PIVOT_FRACTION (a pivot at or below it
zeroes its column of L and its entry of rho, L rho = b), the landmark's three Jacobian rows a replaced by L^T a and its
residuals by rho, and the pivot of the wrist increment at the weighted centroid of the START's landmarks.
`fit_views(..., dtype=np.float64)` is the oracle, `dtype=np.float32` the same code in float32 - with numpy's LU solve or
step_cases.cholesky_solve (`solver`)."""
import functools
import os

import numpy as np

import fit_cases as fc
import info_cases as ic
import mesh_cases as mc
import step_cases as st
import triangulate_cases as tc

CONVERGED, AT_MAX_ITERS, REFUSED = fc.CONVERGED, fc.AT_MAX_ITERS, fc.REFUSED


# ----------------------------------------------------------------------------- the observations
class Views:
    """The observations of B poses as the kernel reads them.  window [B,V,21,2], cam_rows [B,V], table [R,32|24], weights
    [B,V,21] float32 or None.  used [B,V,21]; refused [B]; w [B,V,21] float64, 0 where unused; wl [B,21] = sum_v w in `dtype`."""

    def __init__(self, window, cam_rows, table, weights, dtype):
        window, table, rows = np.asarray(window, np.float64), np.asarray(table, np.float64), np.asarray(cam_rows)
        b, v_max = window.shape[:2]
        if not 1 <= v_max <= tc.MAX_VIEWS or window.shape[2:] != (21, 2) or table.shape[1] not in (24, 32):
            raise ValueError("bad argument")
        if ((rows < -1) | (rows >= table.shape[0])).any():
            raise IndexError("cam_rows outside [-1, n_rows)")
        self.kind = tc.FISHEYE62 if table.shape[1] == 32 else tc.PINHOLE
        self.tab = table[np.maximum(rows, 0)]                                  # [B,V,32|24]
        w_in = np.ones((b, v_max, 21)) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
        seen = np.broadcast_to((rows >= 0)[..., None], (b, v_max, 21))
        with np.errstate(all="ignore"):
            w_ok = np.isfinite(w_in) & (w_in > 0)
            bad_w = seen & ~(np.isfinite(w_in) & (w_in >= 0))
            win_ok = np.isfinite(window).all(-1)
            bad_win = seen & w_ok & ~win_ok
        self.used = seen & w_ok & win_ok
        self.w = np.where(self.used, w_in, 0.0)
        self.window = np.where(self.used[..., None], window, 0.0)
        wl = np.zeros((b, 21), dtype)
        for v in range(v_max):
            wl = wl + self.w[:, v].astype(dtype)
        self.wl = wl
        self.refused = bad_w.any((1, 2)) | bad_win.any((1, 2)) | (self.used.any(1).sum(1) < 3) | ~np.isfinite(wl).all(1)
        self.v_max = v_max

    def blocks(self, p, idx):
        """Poses idx at landmarks p [len(idx),21,3] (any dtype; projected in float64), views ascending: per landmark cost
        [k,21], M = (a00, a10, a11, a20, a21, a22), b = (b0, b1, b2), good [k,21] (finite, and behind no used pinhole view's near
        plane), squared reprojection distance [k,V,21], and per view the residual [k,21,2] and the Jacobian [k,21,2,3] (0
        where unused)."""
        x = np.asarray(p, np.float64)
        k = len(idx)
        cost = np.zeros((k, 21))
        m = [np.zeros((k, 21)) for _ in range(6)]
        g = [np.zeros((k, 21)) for _ in range(3)]
        good = np.ones((k, 21), bool)
        sq_all = np.zeros((k, self.v_max, 21))
        res, jacs = [], []
        with np.errstate(all="ignore"):
            for v in range(self.v_max):
                u = self.used[idx, v]
                win, ez, jac = tc.project(self.tab[idx, v, None, :], x, self.kind, jacobian=True)
                r = np.where(u[..., None], win - self.window[idx, v], 0.0)
                jac = np.where(u[..., None, None], jac, 0.0)
                wv = self.w[idx, v]
                if self.kind == tc.PINHOLE:
                    good &= ~(u & ~(ez >= tc.NEAR_Z))
                sq = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
                sq_all[:, v] = sq
                cost = cost + wv * sq
                n = 0
                for a in range(3):
                    for c in range(a + 1):
                        m[n] = m[n] + wv * (jac[..., 0, a] * jac[..., 0, c] + jac[..., 1, a] * jac[..., 1, c])
                        n += 1
                    g[a] = g[a] + wv * (jac[..., 0, a] * r[..., 0] + jac[..., 1, a] * r[..., 1])
                res.append(r)
                jacs.append(jac)
            good &= np.isfinite(cost)
        return cost, m, g, good, sq_all, res, jacs

    def cost(self, p, idx, dtype):
        """(cost [k] in dtype: per landmark in float64, rounded once, summed - +inf where a used observation cannot be projected;
        the largest reprojection distance [k] in dtype; the distances [k,V,21])."""
        cost, _m, _g, good, sq, _r, _j = self.blocks(p, idx)
        any_used = self.used[idx].any(1)
        with np.errstate(all="ignore"):
            c = np.where(any_used, np.where(good, cost.astype(dtype), dtype(np.inf)), dtype(0))
            far = np.where(any_used & good, np.where(self.used[idx], sq, 0.0).max(1).astype(dtype), dtype(0))
            return c.sum(1, dtype=dtype), np.sqrt(far.max(1)), np.sqrt(np.where(self.used[idx], sq, 0.0))


def semidefinite_cholesky(m, g):
    """M = L L^T and L rho = b per landmark: (factor [...,6] = l00 l10 l11 l20 l21 l22, rho [...,3]).  A pivot at or below
    tc.PIVOT_FRACTION x the largest diagonal entry zeroes its column of L and its entry of rho."""
    a00, a10, a11, a20, a21, a22 = m
    with np.errstate(all="ignore"):
        floor = tc.PIVOT_FRACTION * np.maximum(a00, np.maximum(a11, a22))
        k0 = a00 > floor
        l00 = np.where(k0, np.sqrt(np.where(k0, a00, 1.0)), 0.0)
        s00 = np.where(k0, l00, 1.0)
        l10, l20, r0 = np.where(k0, a10 / s00, 0.0), np.where(k0, a20 / s00, 0.0), np.where(k0, g[0] / s00, 0.0)
        p1 = a11 - l10 * l10
        k1 = p1 > floor
        l11 = np.where(k1, np.sqrt(np.where(k1, p1, 1.0)), 0.0)
        s11 = np.where(k1, l11, 1.0)
        l21, r1 = np.where(k1, (a21 - l20 * l10) / s11, 0.0), np.where(k1, (g[1] - l10 * r0) / s11, 0.0)
        p2 = (a22 - l20 * l20) - l21 * l21
        k2 = p2 > floor
        l22 = np.where(k2, np.sqrt(np.where(k2, p2, 1.0)), 0.0)
        r2 = np.where(k2, ((g[2] - l20 * r0) - l21 * r1) / np.where(k2, l22, 1.0), 0.0)
    return np.stack([l00, l10, l11, l20, l21, l22], -1), np.stack([r0, r1, r2], -1)


def reduced_system(vw, sub, ang, m, centroid, idx, dtype):
    """The 63 rows the solver sees for poses idx: (J [k,63,26], r [k,63]) in dtype - the landmark's Jacobian rows a replaced
    by L^T a and its residuals by rho."""
    k = len(idx)
    p = fc.forward(sub, ang, m, dtype)
    _c, mm, g, _good, _sq, _r, _j = vw.blocks(p, idx)
    f, rho = semidefinite_cholesky(mm, g)
    any_used = vw.used[idx].any(1)
    f = np.where(any_used[..., None], f, 0.0).astype(dtype)
    rho = np.where(any_used[..., None], rho, 0.0).astype(dtype)
    jac = fc.jacobian(sub, ang, m, centroid, dtype).reshape(k, 21, 3, 26)
    jac = ic.whiten(f, np.where(any_used[..., None, None], jac, dtype(0))).reshape(k, 63, 26)
    return jac, rho.reshape(k, 63)


def stacked_system(vw, sub, ang, m, centroid, idx):
    """The full Gauss-Newton system in float64, 2 V 21 rows: (J [k,V*21*2,26], r [k,V*21*2]), rows weighted by sqrt(w)."""
    k = len(idx)
    p = fc.forward(sub, ang, m, np.float64)
    _c, _m, _g, _good, _sq, res, jacs = vw.blocks(p, idx)
    jl = fc.jacobian(sub, ang, m, centroid, np.float64).reshape(k, 21, 3, 26)
    rows_j, rows_r = [], []
    for v in range(vw.v_max):
        sw = np.sqrt(vw.w[idx, v])
        rows_j.append((sw[..., None, None] * (jacs[v] @ jl)).reshape(k, 42, 26))
        rows_r.append((sw[..., None] * res[v]).reshape(k, 42))
    return np.concatenate(rows_j, 1), np.concatenate(rows_r, 1)


def pivot(vw, p, dtype):
    """(centroid [B,3], extent [B], wsum [B]) of landmarks p with the weights sum_v w_vl; weights 1 for refused poses."""
    w = np.where(vw.refused[:, None], dtype(1), vw.wl).astype(dtype)
    wsum = w.sum(1)
    with np.errstate(all="ignore"):
        centroid = (w[..., None] * p).sum(1) / wsum[:, None]
        extent = np.sqrt((w * ((p - centroid[:, None]) ** 2).sum(-1)).sum(1) / wsum)
    return centroid, extent, wsum


# ----------------------------------------------------------------------------- the fit
class _Reprojection(fc.Problem):
    """fc.Problem on the observations vw (Views): no targets, so no cold start, and the pivot, the extent and the sum of the
    weights are those of the START's landmarks (pivot).  residual [B,V,21] float32 after the fit."""

    def __init__(self, hm, dtype, vw):
        self.hm, self.dt, self.vw, self.refused = hm, dtype, vw, vw.refused

    def _cost(self, idx, ang, m):
        with np.errstate(all="ignore"):
            return self.vw.cost(fc.forward(fc._take(self.hm, idx), ang, m, self.dt), idx, self.dt)

    def pivot(self, ang, m):
        with np.errstate(all="ignore"):
            return pivot(self.vw, fc.forward(self.hm, ang, m, self.dt), self.dt)

    def system(self, idx, ang, m, centroid):
        return reduced_system(self.vw, fc._take(self.hm, idx), ang, m, centroid, idx, self.dt)

    def cost(self, idx, ang, m, extra=None):
        return self._cost(idx, ang, m)[:2]

    def report(self, refused, ang, m, centroid, status):
        residual = self._cost(np.arange(len(refused)), ang, m)[2]
        self.residual = np.where(refused[:, None, None], 0.0, residual).astype(np.float32)
        return []


def fit_views(hm, window, cam_rows, table, weights=None, init=None, mirror=None, limits=None, t_scale=1.0, max_iters=32,
              dtype=np.float64, solver="lu", trace=None):
    """ut_fit_pose_views: (joint_angles [B,22], wrist_xf [B,4,4], info [B,4]: sqrt(cost / sum of the used weights), the largest
    reprojection distance of a used observation, iterations, status; residual [B,V,21]: the reprojection distance of every used
    observation at the returned pose).  init = (joint_angles [B,22], wrist_xf [B,4,4]) is required.  Refused: a negative or
    non-finite weight of a seen view, a non-finite window at a positive weight, fewer than 3 landmarks with a used observation
    (the start comes back), a start whose cost is not finite (the rest pose at the identity comes back, as fc.fit does)."""
    if init is None:
        raise ValueError("init is required: there is no cold start")
    prob = _Reprojection(hm, dtype, Views(window, cam_rows, table, weights, dtype))
    with st.solver(solver):
        return fc.lm(prob, limits, init, mirror, t_scale, max_iters, trace=trace) + (prob.residual,)


# ----------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def golden():
    """ic.golden_hands() with the label poses of its 74 hands (ja, xf), the two cameras that see most of each hand in
    ascending order (`seeing` [74,2]) and the one that sees most (`best` [74,1]).  Cached: leave it unchanged."""
    from absolutetrack_amd import pipeline
    g = ic.golden_hands()
    z = np.load(os.path.join(tc.GOLDEN, "projection_rec00.npz"))
    ja, xf, hand = mc.label_poses(pipeline.load_labels())
    sel = 2 * z["frame"][z["case_frame"]] + z["hand"]
    assert np.array_equal(hand[sel], g["hand"]) and set(g["hand"]) == {0, 1}
    g["ja"], g["xf"] = ja[sel], xf[sel]
    order = np.argsort(-g["weights"].sum(2), axis=1, kind="stable")
    g["seeing"], g["best"] = np.sort(order[:, :2], 1), order[:, :1]
    assert np.all(np.take_along_axis(g["weights"].sum(2), g["seeing"], 1) >= 3)
    return g


def select(g, cols, window=None):
    """Views `cols` [74,k] of the golden hands: dict(window [74,k,21,2], cam_rows [74,k], weights [74,k,21])."""
    win = g["window"] if window is None else window
    return dict(window=np.take_along_axis(win, cols[:, :, None, None], 1).copy(),
                cam_rows=np.take_along_axis(g["cam_rows"], cols, 1).astype(np.int32),
                weights=np.take_along_axis(g["weights"], cols[:, :, None], 1).astype(np.float32))


def starts(g, seed, angle, shift):
    """The label poses plus uniform noise: +-angle rad on the 20 angles and on the wrist's rotation vector, +-shift mm; float32."""
    return st.perturbed(g["ja"], g["xf"], seed, angle, angle, shift)


def posed(g, hm):
    """The float64 landmarks of the 74 label poses on skeleton hm."""
    return fc.forward(hm, g["ja"][:, :20], fc.effective_wrist(g["xf"], g["hand"], 1.0, np.float64))


def exact_windows(table, cam_rows, landmarks):
    """Landmarks [n,21,3] through the cameras cam_rows [n,k] of table (a -1 row gives 0): [n,k,21,2]."""
    kind = tc.FISHEYE62 if table.shape[1] == 32 else tc.PINHOLE
    tab = table[np.maximum(cam_rows, 0)]
    win = np.stack([tc.project(tab[:, v, None, :], landmarks, kind)[0] for v in range(cam_rows.shape[1])], 1)
    return np.where((cam_rows >= 0)[:, :, None, None], win, 0.0)


STEP_CASES = ("two_views", "best_view", "ragged", "spread", "pinhole", "metres", "table_a", "table_b", "mixed")


def ragged(c, seed=5):
    """A two-view case made ragged, on three view slots: the second view misses 12 random landmarks (weight 0); every third
    pose has its views in slots 0 and 2 with a -1 hole between them; one of the weight-0 observations of every pose has a NaN
    window."""
    rng = np.random.default_rng(seed)
    n = len(c["cam_rows"])
    win = np.zeros((n, 3, 21, 2))
    rows = np.full((n, 3), -1, np.int32)
    w = np.zeros((n, 3, 21), np.float32)
    second = np.where(np.arange(n) % 3 == 1, 2, 1)
    for i in range(n):
        miss = rng.choice(21, 12, replace=False)
        win[i, 0], rows[i, 0], w[i, 0] = c["window"][i, 0], c["cam_rows"][i, 0], c["weights"][i, 0]
        win[i, second[i]], rows[i, second[i]], w[i, second[i]] = c["window"][i, 1], c["cam_rows"][i, 1], c["weights"][i, 1]
        w[i, second[i], miss] = 0
        win[i, second[i], miss[0]] = np.nan
    return dict(c, window=win, cam_rows=rows, weights=w)


@functools.lru_cache(maxsize=None)
def case(name):
    """The one-step case `name` on the 74 golden hands: dict(hm, window, cam_rows, table, weights, init, mirror, t_scale, limits,
    truth = the float64 landmarks behind the windows).  Exact windows of the label poses on the case's skeleton; starts
    +-0.2 rad / +-15 mm (seed 31), float32.  Cached: leave it unchanged."""
    g = golden()
    n = len(g["hand"])
    hm = st.skeleton({"table_a": "a", "table_b": "b", "mixed": "mixed"}[name], n) if name in ("table_a", "table_b", "mixed") else g["hm"]
    truth = posed(g, hm)
    table = tc.pinhole_from_fisheye(g["table"]) if name == "pinhole" else g["table"]
    c = select(g, g["best"] if name == "best_view" else g["seeing"])
    c["window"] = exact_windows(table, c["cam_rows"], truth)
    ja0, xf0 = starts(g, 31, 0.2, 15.0)
    t_scale = 1000.0 if name == "metres" else 1.0
    xf0 = xf0.copy()
    xf0[:, :3, 3] = (xf0[:, :3, 3].astype(np.float64) / t_scale).astype(np.float32)
    c.update(hm=hm, table=table, init=(ja0, xf0), mirror=g["hand"], t_scale=t_scale, limits=None, truth=truth)
    if name == "ragged":
        c = ragged(c)
    if name == "spread":
        c["weights"] = (c["weights"] * 10.0 ** np.random.default_rng(47).uniform(-1, 1, c["weights"].shape)).astype(np.float32)
    return c


def subset(c, sel):
    sel = np.asarray(sel)
    out = dict(c, hm=fc._take(c["hm"], sel), init=(c["init"][0][sel], c["init"][1][sel]))
    for k in ("window", "cam_rows", "weights", "mirror", "truth"):
        out[k] = c[k][sel]
    return out


def restate(c, dtype=np.float64, max_iters=1, solver="lu", trace=None):
    """fit_views on a case: dict(ja, xf, info, residual)."""
    ja, xf, info, residual = fit_views(c["hm"], c["window"], c["cam_rows"], c["table"], c["weights"], c["init"], c["mirror"],
                                       c["limits"], c["t_scale"], max_iters, dtype, solver, trace)
    return dict(ja=ja, xf=xf, info=info, residual=residual)


def landmarks(c, res):
    """The float64 forward function of a result on the case's skeleton, in the cameras' world."""
    m = fc.effective_wrist(np.asarray(res["xf"], np.float64), c["mirror"], c["t_scale"], np.float64)
    return fc.forward(c["hm"], np.asarray(res["ja"], np.float64)[:, :20], m, np.float64)


def distance(c, a, b):
    """How far two results of a case lie apart.  ang: the 20 angles modulo 2 pi and the entries of the wrist's rotation, rad.
    kp: landmarks through the float64 forward function of both, mm.  px: rms / worst of info."""
    ia, ib = np.asarray(a["info"], np.float64), np.asarray(b["info"], np.float64)
    return dict(ang=st.angle_and_rotation_distance(a, b), kp=float(np.linalg.norm(landmarks(c, a) - landmarks(c, b), axis=-1).max()),
                px=float(np.abs(ia[:, :2] - ib[:, :2]).max()))


def float32_distance(c, want, max_iters=1):
    """The worst distance of the float32 restatements - one per solver of st.SOLVERS - from the float64 result `want`."""
    return st.worst([distance(c, restate(c, np.float32, max_iters, s), want) for s in st.SOLVERS])


def bounds_from(d32):
    """DESIGN's rule for one step against float64: the project's bounds where float32 stays within a quarter of them, else
    st.FLOAT32_FACTOR x the float32 restatement's own distance.  px (rms and worst of info) has no project bound: the factor
    alone, and never below what rounding the float64 figure to float32 costs at 300 px (2^-23 x 300)."""
    return dict(ang=max(st.ANGLE_TOL_RAD, st.FLOAT32_FACTOR * d32["ang"]), kp=max(st.KP_TOL_MM, st.FLOAT32_FACTOR * d32["kp"]),
                px=max(300.0 * 2.0 ** -23, st.FLOAT32_FACTOR * d32["px"]))


within = st.within


# ----------------------------------------------------------------------------- full fits
FULL_SEED, FULL_DRAWS = 31, 8
BASIN_MM = 1.0            # a float32 fit this close to the hand sits in the hand's basin: the other basins lie tens of mm away


@functools.lru_cache(maxsize=None)
def full_case(views):
    """The reference's own windows of the 74 hands in their two seeing views ('two') or the best view alone ('one'); starts
    +-0.4 rad on the 20 angles and +-30 mm on the wrist (st.perturbed, seed FULL_SEED); truth = the golden landmarks.

    One view leaves a finger free to fold towards the camera or away from it with nearly the same picture: from +-0.4 rad a few
    starts lie in the basin of such a mirror pose, a stationary point of the cost itself (seed 31: hand 14, the little finger
    16 mm off at 0.08 px rms; hand 25, the thumb 113 mm off at 0.55 px), where every correct solver ends.  Which basin a start
    lies in is a property of the cost and the draw, not of the code under test, so - as step_cases.rejected_case selects its
    starts by the restatements' decisions - a hand whose start the restatements of st.RUNS do not all take to the hand (float64
    within st.KP_TOL_MM, float32 within BASIN_MM) draws again with the next seed, up to FULL_DRAWS draws.  `draws` [74] is the
    number of draws each hand took; with two views every hand keeps its first.  Cached: leave it unchanged."""
    g = golden()
    c = select(g, g["seeing"] if views == "two" else g["best"])
    c.update(hm=g["hm"], table=g["table"], mirror=g["hand"], t_scale=1.0, limits=None, truth=g["landmarks"].astype(np.float64))
    n = len(g["hand"])
    ja0, xf0 = (a.copy() for a in st.perturbed(g["ja"], g["xf"], FULL_SEED, 0.4, 0.0, 30.0))
    draws, todo = np.ones(n, np.int64), np.arange(n)
    for k in range(FULL_DRAWS):
        if k:
            ja_k, xf_k = st.perturbed(g["ja"], g["xf"], FULL_SEED + k, 0.4, 0.0, 30.0)
            ja0[todo], xf0[todo] = ja_k[todo], xf_k[todo]
            draws[todo] += 1
        part = subset(dict(c, init=(ja0, xf0)), todo)
        ok = np.ones(len(todo), bool)
        for dt, how in st.RUNS:
            r = restate(part, dt, 32, how)
            err = np.linalg.norm(landmarks(part, r) - part["truth"], axis=-1).max(1)
            ok &= (r["info"][:, 3] == CONVERGED) & (err <= (st.KP_TOL_MM if dt is np.float64 else BASIN_MM))
        todo = todo[~ok]
        if not len(todo):
            break
    assert not len(todo), (views, todo)
    c.update(init=(ja0, xf0), draws=draws)
    return c


@functools.lru_cache(maxsize=None)
def full_yardstick(views):
    """Full fits (max_iters = 32) of full_case(views) by the restatements of st.RUNS, which must converge on every pose:
    (float32 iterations [n] - the larger of the two float32 runs -, float64 iterations [n], margin = the largest distance of a
    float32 count from the float64 one, at least 2, the three results)."""
    c = full_case(views)
    runs = [restate(c, dt, 32, how) for dt, how in st.RUNS]
    for r in runs:
        assert np.all(r["info"][:, 3] == CONVERGED), views
    its = [r["info"][:, 2].astype(np.int64) for r in runs]
    both = np.stack(its[:2])
    return both.max(0), its[2], max(2, int(np.abs(both - its[2]).max())), runs


@functools.lru_cache(maxsize=None)
def noisy_ragged():
    """1 px detection noise (seed 0) on the two seeing views, the second view missing 12 random landmarks (weight 0): the case,
    with init = the float64 chain ic.chain (triangulation with factor -> isotropic fit -> information fit) on the landmarks two
    views still see, rounded to float32.  Cached: leave it unchanged."""
    g = golden()
    c = select(g, g["seeing"], ic.noisy_windows(g, 1.0, 0))
    rng = np.random.default_rng(11)
    for i in range(len(c["weights"])):
        c["weights"][i, 1, rng.choice(21, 12, replace=False)] = 0
    ch = ic.chain(dict(g, window=c["window"], cam_rows=c["cam_rows"], weights=c["weights"]), c["window"])
    c.update(hm=g["hm"], table=g["table"], init=(ch["info"][0].astype(np.float32), ch["info"][1].astype(np.float32)), mirror=g["hand"],
             t_scale=1.0, limits=None, truth=g["landmarks"].astype(np.float64), chain=ch)
    return c
