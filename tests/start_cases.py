"""Shared by tests/test_start_host.py, tests/test_gpu_start.py and tools/bench_start.py: the numpy restatement of
ut_start_pose_views and ut_select_pose (include/umetrack_hip_start.h, csrc/start_views.hip) and the cases their tests share.

`start_pose_views` takes the kernel's decisions: fit_views' rules for used observations and refusals (views_cases.Views), the
rays of triangulate_cases.unproject, the rigid shape = the float32 landmarks of the clamped bank pose under the identity wrist
(column 0 negated for a mirrored hand, as fit_cases.cold_start), the translation in closed form, the rotation by numpy's SVD
with the determinant fix, `iters` rounds and the translation once more, the score through triangulate_cases.project.
dtype=np.float64 is the oracle; dtype=np.float32 runs the iteration itself (R, t, the correlation, the SVD) in float32 - the
twin whose distance from the oracle says what float32 would cost; rays, shape and score stay float64 in both."""
import functools

import numpy as np

import fit_cases as fc
import step_cases as st
import triangulate_cases as tc
import views_cases as vc

REFUSED = fc.REFUSED
ITERS = 30
FLOAT32_FACTOR = st.FLOAT32_FACTOR
BASIN_MM = 5.0            # the selected pose's worst landmark this close to the golden landmarks: the hand's basin was found
FRACTIONS = (0.25, 0.5, 0.75)


def bank(limits=None, fractions=FRACTIONS):
    """hand.start_pose_bank: the zero pose, then lo + f (hi - lo) of limits [20,2]; float32 [K,20]."""
    limits = st.joint_limits() if limits is None else limits
    rows = [np.zeros(20, np.float32)] + [(limits[:, 0] + np.float32(f) * (limits[:, 1] - limits[:, 0])).astype(np.float32) for f in fractions]
    return np.stack(rows)


def seeds():
    """hand.start_rotation_seeds: the 24 proper signed permutation matrices [24,3,3]."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        parity = 1.0 if perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1.0
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                q = np.zeros((3, 3))
                q[0, perm[0]], q[1, perm[1]], q[2, perm[2]] = s0, s1, parity * s0 * s1
                out.append(q)
    return np.stack(out)


def rigid_shape(hm, angles, mirror, dtype=np.float32):
    """Landmarks [B,21,3] (float64 values of the `dtype` forward function) of angles [B,20] under the identity wrist, column 0
    negated where mirror == 1."""
    b = angles.shape[0]
    eye = np.tile(np.eye(4, dtype=dtype), (b, 1, 1))
    if mirror is not None:
        eye[np.asarray(mirror) == 1, 0, 0] = -1
    return fc.forward(hm, angles.astype(dtype), eye, dtype).astype(np.float64)


def factor_is_regular(m):
    """csrc/ut_camera.h's chol3 on M [B,3,3] with the floor PIVOT_FRACTION x the largest diagonal entry: [B] bool."""
    with np.errstate(all="ignore"):
        floor = tc.PIVOT_FRACTION * np.maximum(m[:, 0, 0], np.maximum(m[:, 1, 1], m[:, 2, 2]))
        l00 = np.sqrt(m[:, 0, 0])
        l10, l20 = m[:, 1, 0] / l00, m[:, 2, 0] / l00
        p1 = m[:, 1, 1] - l10 * l10
        l21 = (m[:, 2, 1] - l20 * l10) / np.sqrt(p1)
        p2 = (m[:, 2, 2] - l20 * l20) - l21 * l21
        return (m[:, 0, 0] > floor) & (p1 > floor) & (p2 > floor) & np.isfinite(m[:, 0, 0] + p1 + p2)


class Rays:
    """The used observations of B hands as rays: w [B,O] (0 = unused), o, d [B,O,3], lm [O] landmark of slot O = V * 21, views
    ascending; m = sum w A [B,3,3]; refused [B] (fit_views' rules, or a singular m); first [B]: the first view with a used
    observation; rot [B,3,3]: its eye -> world rotation."""

    def __init__(self, window, cam_rows, table, weights):
        self.vw = vw = vc.Views(window, cam_rows, table, weights, np.float32)
        b, v = vw.used.shape[:2]
        with np.errstate(all="ignore"):
            o, d = tc.unproject(vw.tab[:, :, None, :], vw.window, vw.kind)
        self.w = vw.w.reshape(b, v * 21)
        self.o = np.broadcast_to(o, (b, v, 21, 3)).reshape(b, v * 21, 3)
        self.d = np.where(vw.used[..., None], d, 0.0).reshape(b, v * 21, 3)
        self.lm = np.tile(np.arange(21), v)
        a = np.eye(3) - self.d[..., :, None] * self.d[..., None, :]
        self.m = (self.w[..., None, None] * a).sum(1)
        self.refused = vw.refused | ~factor_is_regular(np.where(vw.refused[:, None, None], np.eye(3), self.m))
        self.first = np.argmax(vw.used.any(2), 1)
        rot = tc._split(vw.tab, vw.kind)[2]
        self.rot = rot[np.arange(b), self.first]

    def translation(self, rp, ok):
        """t [B,S,3] = -(sum w A)^-1 sum w A (R p - o) for rp = R p [B,S,O,3], in rp's dtype."""
        dt = rp.dtype
        y = rp - self.o[:, None].astype(dt)
        d = self.d[:, None].astype(dt)
        ay = y - d * (d * y).sum(-1, keepdims=True)
        rhs = (self.w[:, None, :, None].astype(dt) * ay).sum(2)
        m = np.where(ok[:, None, None], self.m, np.eye(3)).astype(dt)
        return -np.linalg.solve(m[:, None], rhs[..., None])[..., 0]


def iterate(rays, p, rot0, iters, dtype=np.float64):
    """The orthogonal iteration from rot0 [B,S,3,3] on the shape p [B,21,3]: (R [B,S,3,3], t [B,S,3]) in dtype."""
    ok = ~rays.refused
    w = rays.w.astype(dtype)
    po = p[:, rays.lm].astype(dtype)                                    # [B,O,3]
    wsum = np.where(ok, w.sum(1), 1)
    pc = (w[..., None] * po).sum(1) / wsum[:, None]
    pt = po - pc[:, None]
    d = rays.d[:, None].astype(dtype)
    r = rot0.astype(dtype)
    with np.errstate(all="ignore"):
        for _ in range(iters):
            rp = np.einsum("bsij,boj->bsoi", r, po)
            t = rays.translation(rp, ok)
            z = rp + t[:, :, None] - rays.o[:, None].astype(dtype)
            az = z - d * (d * z).sum(-1, keepdims=True)
            foot = np.einsum("bsij,boj->bsoi", r, pt) - az               # the foot point minus the constant R pc + t
            h = np.einsum("bo,boi,bsoj->bsij", w, pt, foot)
            h = np.where(np.isfinite(h).all((-2, -1), keepdims=True), h, 0)
            u, _s, vt = np.linalg.svd(h.astype(dtype))
            v, ut = np.swapaxes(vt, -1, -2), np.swapaxes(u, -1, -2)
            fix = np.tile(np.eye(3, dtype=dtype), h.shape[:2] + (1, 1))
            fix[..., 2, 2] = np.sign(np.linalg.det((v @ ut).astype(np.float64)))
            r = (v @ fix @ ut).astype(dtype)
        t = rays.translation(np.einsum("bsij,boj->bsoi", r, po), ok)
    return r, t


def score(rays, p, r, t):
    """The squared cost of the fit in the views at R p + t, float64: (cost [B,S], +inf where a used observation cannot be
    projected or crosses NEAR_Z of a used pinhole view; the largest squared reprojection distance [B,S])."""
    vw = rays.vw
    b, v = vw.used.shape[:2]
    x = np.einsum("bsij,blj->bsli", r.astype(np.float64), p) + t.astype(np.float64)[:, :, None]
    cost = np.zeros(x.shape[:2])
    far = np.zeros(x.shape[:2])
    good = np.ones(x.shape[:2], bool)
    with np.errstate(all="ignore"):
        for k in range(v):
            win, ez = tc.project(vw.tab[:, None, k, None, :], x, vw.kind)
            u = vw.used[:, None, k]
            res = np.where(u[..., None], win - vw.window[:, None, k], 0.0)
            sq = res[..., 0] * res[..., 0] + res[..., 1] * res[..., 1]
            if vw.kind == tc.PINHOLE:
                good &= ~(u & ~(ez >= tc.NEAR_Z)).any(-1)
            cost = cost + (vw.w[:, None, k] * sq).sum(-1)
            far = np.maximum(far, sq.max(-1))
        good &= np.isfinite(cost)
    return np.where(good, cost, np.inf), far


def start_pose_views(hm, window, cam_rows, table, bank_angles, seed_rot, weights=None, mirror=None, limits=None, t_scale=1.0,
                     iters=ITERS, dtype=np.float64):
    """ut_start_pose_views: dict(ja [B K,22] float32, xf [B K,4,4] float32, info [B K,4] float32, cost and rms [B,K,S] float64 - every
    seed's score and sqrt(score / sum of the used weights) -, landmarks [B K,21,3] float64 of the start in the cameras' world, 0 for refused rows)."""
    rays = Rays(window, cam_rows, table, weights)
    b, k_n, s_n = len(rays.refused), len(bank_angles), len(seed_rot)
    ja = np.zeros((b, k_n, 22), np.float32)
    xf = np.tile(np.eye(4, dtype=np.float32), (b, k_n, 1, 1))
    info = np.zeros((b, k_n, 4), np.float32)
    costs = np.full((b, k_n, s_n), np.inf)
    lms = np.zeros((b, k_n, 21, 3))
    rot0 = np.einsum("bij,sjk->bsik", rays.rot, np.asarray(seed_rot, np.float64))
    wsum = np.where(rays.refused, 1.0, rays.w.sum(1))
    for k in range(k_n):
        ang = np.tile(np.asarray(bank_angles[k], np.float32), (b, 1))
        if limits is not None:
            box = np.broadcast_to(np.asarray(limits, np.float32).reshape(-1, 20, 2), (b, 20, 2)) if np.asarray(limits).reshape(-1, 20, 2).shape[0] == 1 \
                else np.asarray(limits, np.float32).reshape(b, 20, 2)
            ang = np.minimum(np.maximum(ang, box[..., 0]), box[..., 1])
        ja[:, k, :20] = ang
        p = rigid_shape(hm, ang, mirror)
        r, t = iterate(rays, p, rot0, iters, dtype)
        c, far = score(rays, p, r, t)
        c = np.where(rays.refused[:, None], np.inf, c)
        costs[:, k] = c
        win = np.argmin(c, 1)
        pick = np.arange(b)
        ok = np.isfinite(c[pick, win])
        rw, tw = r[pick, win].astype(np.float64), t[pick, win].astype(np.float64)
        xf[ok, k, :3, :3] = rw[ok].astype(np.float32)
        xf[ok, k, :3, 3] = tw[ok].astype(np.float32) / np.float32(t_scale)
        with np.errstate(all="ignore"):
            info[:, k, 0] = np.where(ok, np.sqrt(np.where(ok, c[pick, win], 0.0) / wsum), 0.0)
            info[:, k, 1] = np.where(ok, np.sqrt(far[pick, win]), 0.0)
        info[:, k, 2] = np.where(ok, win, -1)
        info[:, k, 3] = np.where(ok, 0, REFUSED)
        lms[ok, k] = (np.einsum("bij,blj->bli", rw, p) + tw[:, None])[ok]
    with np.errstate(all="ignore"):
        rms = np.sqrt(costs / wsum[:, None, None])
    return dict(ja=ja.reshape(b * k_n, 22), xf=xf.reshape(b * k_n, 4, 4), info=info.reshape(b * k_n, 4), cost=costs, rms=rms,
                landmarks=lms.reshape(b * k_n, 21, 3))


def select_pose(ja, xf, info, n_cand):
    """ut_select_pose: (ja [n,22], xf [n,4,4], info [n,4], index int32 [n])."""
    ja, xf, info = np.asarray(ja, np.float32).reshape(-1, n_cand, 22), np.asarray(xf, np.float32).reshape(-1, n_cand, 4, 4), \
        np.asarray(info, np.float32).reshape(-1, n_cand, 4)
    n = len(info)
    index = np.full(n, -1, np.int32)
    for i in range(n):
        best = np.float32(0)
        for c in range(n_cand):
            if int(info[i, c, 3]) & REFUSED:
                continue
            if index[i] < 0 or info[i, c, 0] < best or (np.isnan(best) and not np.isnan(info[i, c, 0])):
                index[i], best = c, info[i, c, 0]
    src = np.maximum(index, 0)
    pick = np.arange(n)
    return ja[pick, src], xf[pick, src], info[pick, src], index


def repeat_case(c, k):
    """Every hand of a views case k times in a row: what the fit on the n k starts reads."""
    out = dict(c, hm=c["hm"] if np.asarray(c["hm"]["landmark_rest_positions"]).ndim == 2 else {f: np.repeat(np.asarray(a), k, 0) for f, a in c["hm"].items()})
    for f in ("window", "cam_rows", "weights", "mirror"):
        out[f] = None if c[f] is None else np.repeat(c[f], k, 0)
    return out


def cold_fit(c, bank_angles=None, seed_rot=None, iters=ITERS, max_iters=64, dtype=np.float64, starts=None):
    """The chain on a views case (dict(hm, window, cam_rows, table, weights, mirror, limits, t_scale)): the starts (or `starts`,
    dict(ja, xf) of another source), views_cases.fit_views from each, select_pose.  dict(ja, xf, info, index, starts, fits)."""
    bank_angles = bank() if bank_angles is None else bank_angles
    seed_rot = seeds() if seed_rot is None else seed_rot
    k = len(bank_angles)
    if starts is None:
        starts = start_pose_views(c["hm"], c["window"], c["cam_rows"], c["table"], bank_angles, seed_rot, c["weights"], c["mirror"],
                                  c["limits"], c["t_scale"], iters)
    r = repeat_case(c, k)
    fits = vc.fit_views(r["hm"], r["window"], r["cam_rows"], r["table"], r["weights"], (starts["ja"], starts["xf"]), r["mirror"], c["limits"],
                        c["t_scale"], max_iters, dtype)
    ja, xf, info, index = select_pose(fits[0], fits[1], fits[2], k)
    return dict(ja=ja, xf=xf, info=info, index=index, starts=starts, fits=fits)


# ----------------------------------------------------------------------------- the yardstick on the 74 golden hands
@functools.lru_cache(maxsize=None)
def golden_case(views, noise):
    """The 74 golden hands in their two seeing views ('two') or the best view alone ('one'), the reference's own windows plus
    `noise` px of default_rng(0) noise; truth = the golden landmarks; label = the label poses (float32).  Cached: leave it
    unchanged."""
    g = vc.golden()
    import info_cases as ic
    c = vc.select(g, g["seeing"] if views == "two" else g["best"], ic.noisy_windows(g, noise, 0) if noise else None)
    c.update(hm=g["hm"], table=g["table"], mirror=g["hand"], t_scale=1.0, limits=None, truth=g["landmarks"].astype(np.float64),
             label=(g["ja"].astype(np.float32), g["xf"].astype(np.float32)))
    return c


def landmark_error(c, res):
    """The worst landmark's distance [n] of a result from the case's truth, mm."""
    return np.linalg.norm(vc.landmarks(c, res) - c["truth"], axis=-1).max(1)


def rms_criterion(c, res, max_iters=64):
    """[n] bool: the result's rms <= 1.05 x the rms of the float64 fit started at the label + 0.01 px."""
    ref = vc.fit_views(c["hm"], c["window"], c["cam_rows"], c["table"], c["weights"], c["label"], c["mirror"], c["limits"], c["t_scale"], max_iters)
    return np.asarray(res["info"], np.float64)[:, 0] <= 1.05 * ref[2][:, 0].astype(np.float64) + 0.01


# ----------------------------------------------------------------------------- the tracker's rule
RECOVER_RATIO, RECOVER_FLOOR_PX = 1.5, 0.01      # tracker.RECOVER_RATIO, tracker.RECOVER_FLOOR_PX


def track(c, cold, init, recover_ratio=RECOVER_RATIO, max_iters=32):
    """tracker.track_hand_poses_in_views on the frames of a views case in float64: frame t is fitted from the previous frame's
    choice (frame 0 from init = (ja [1,22], xf [1,4,4])) and keeps that warm fit unless it is refused or its rms exceeds
    recover_ratio x the cold rms + RECOVER_FLOOR_PX; recover_ratio None never takes the cold result `cold` (cold_fit's).
    dict(ja, xf, info, warm_rms [T], recovered [T])."""
    n = len(c["mirror"])
    ja, xf, info = np.zeros((n, 22), np.float32), np.zeros((n, 4, 4), np.float32), np.zeros((n, 4), np.float32)
    warm_rms, recovered = np.zeros(n), np.zeros(n, bool)
    prev = init
    for t in range(n):
        s = slice(t, t + 1)
        w = vc.fit_views(fc._take(c["hm"], np.arange(t, t + 1)), c["window"][s], c["cam_rows"][s], c["table"], c["weights"][s], prev, c["mirror"][s],
                         c["limits"], c["t_scale"], max_iters)
        warm_rms[t] = w[2][0, 0]
        lost = (int(w[2][0, 3]) & REFUSED) != 0 or w[2][0, 0] > (recover_ratio or 0) * cold["info"][t, 0] + RECOVER_FLOOR_PX
        recovered[t] = recover_ratio is not None and lost and cold["index"][t] >= 0
        if recovered[t]:
            ja[t], xf[t], info[t] = cold["ja"][t], cold["xf"][t], cold["info"][t]
        else:
            ja[t], xf[t], info[t] = np.asarray(w[0][0], np.float32), np.asarray(w[1][0], np.float32), w[2][0]
        prev = (ja[s], xf[s])
    return dict(ja=ja, xf=xf, info=info, warm_rms=warm_rms, recovered=recovered)
