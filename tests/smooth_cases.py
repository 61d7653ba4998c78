"""Shared by tests/test_smooth_host.py, tests/test_gpu_smooth.py and tools/bench_smooth.py: the numpy restatements of
ut_smooth_pose_sequence (include/umetrack_hip_smooth.h, csrc/smooth.hip) and the sequences its tests share.

`smooth(seq)` is the oracle: the float64 DENSE solve of the 26 T x 26 T block-tridiagonal system and the diagonal blocks of its
inverse.  `smooth(seq, dtype, method)` with method "lu" or "cholesky" is the header's recursion (forward information filter,
backward pass, marginal covariances) in float64 or float32, the linear solves through numpy's LU or through the scaled Cholesky
factor and substitutions, the kernel's algorithm - st.RUNS.  `product=False` is the subtractive M = W - W S^-1 W that the header
warns against; `drop` names what a deliberately wrong restatement leaves out.

A sequence is a dict of what the entry reads, as float32: ja [T,22], xf [T,4,4], pose_info [T,351], pivot [T,3], weight [T] or
None, centre [3] or None, step_var [26], t_scale, and for the distances hm and mirror.  The sequences of recording_00 are built
from pipeline.load_labels(), geometry.pack_source_camera, vc.fit_views and uc.information, restating none of them."""
import functools

import numpy as np

import fit_cases as fc
import mesh_cases as mc
import step_cases as st
import triangulate_cases as tc
import uncertainty_cases as uc
import views_cases as vc

OK, SINGULAR, REFUSED, GAP = 1, 2, 4, 8                  # UT_SMOOTH_*
WORK = 408                                               # UT_SMOOTH_WORK
Q_SCALES = (1e-4, 1e-2, 1.0, 1e2, 1e4)
STEP_SIGMA = (0.02, 0.01, 1.0)                           # rad per angle, rad of rotation, mm of the body point, per frame step


def step_var(angle=STEP_SIGMA[0], rotation=STEP_SIGMA[1], shift=STEP_SIGMA[2]):
    return np.concatenate([np.full(20, angle), np.full(3, rotation), np.full(3, shift)]).astype(np.float32) ** 2


def skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], a.dtype)


def so3_exp(w):
    w = np.asarray(w)
    th = np.sqrt((w * w).sum())
    k = skew(w)
    if th < 1e-4:
        return np.eye(3, dtype=w.dtype) + k + 0.5 * (k @ k)
    return (np.eye(3) + np.sin(th) / th * k + (1 - np.cos(th)) / (th * th) * (k @ k)).astype(w.dtype)


def so3_log(q):
    """The rotation vector of a rotation matrix with an angle below pi: vee of the skew part times theta / sin(theta)."""
    v = 0.5 * np.array([q[2, 1] - q[1, 2], q[0, 2] - q[2, 0], q[1, 0] - q[0, 1]], q.dtype)
    s = np.sqrt((v * v).sum())
    c = 0.5 * (np.trace(q) - 1)
    return v * (1 + s * s / 6 if s < 1e-4 else np.arctan2(s, c) / s)


def wrap(v):
    """Into (-pi, pi], as the fits wrap their angles."""
    v = np.asarray(v)
    return np.where(np.abs(v) > np.pi, v - 2 * np.pi * np.ceil((v - np.pi) / (2 * np.pi)), v)


def bmat(a, inverse=False):
    b = np.eye(26, dtype=a.dtype)
    b[23:26, 20:23] = skew(a) if inverse else -skew(a)
    return b


def prepare(seq, dtype=np.float64, drop=()):
    """What the recursion and the dense solve start from, in dtype: dict(x [T,3] the body point, a [T,3], hp [T,26,26] = H', d
    [T-1,26], w [26], f [T] the weight in force (0 for a gap), refused)."""
    ja, xf = np.asarray(seq["ja"], dtype), np.asarray(seq["xf"], dtype)
    n = len(ja)
    ts = dtype(seq["t_scale"])
    q = np.asarray(seq["step_var"], np.float32)
    with np.errstate(all="ignore"):
        w32 = np.float32(1) / q
    refused = not (np.isfinite(q).all() and (q > 0).all() and np.isfinite(w32).all())
    refused |= not (np.isfinite(ja).all() and np.isfinite(xf[:, :3]).all())
    f = np.ones(n, np.float32) if seq.get("weight") is None or "weight" in drop else np.asarray(seq["weight"], np.float32).copy()
    refused |= not (np.isfinite(f).all() and (f >= 0).all())
    b = np.zeros(3, dtype) if seq.get("centre") is None else np.asarray(seq["centre"], dtype).copy()
    rot, t = xf[:, :3, :3], xf[:, :3, 3] * ts
    x = np.zeros((n, 3), dtype)
    for i in range(n):
        bb = b.copy()
        if np.linalg.det(rot[i].astype(np.float64)) < 0:
            bb[0] = -bb[0]
        x[i] = rot[i] @ bb + t[i]
    refused |= not np.isfinite(x).all()
    hp, a = np.zeros((n, 26, 26), dtype), np.zeros((n, 3), dtype)
    for i in range(n):
        if not f[i] > 0:
            f[i] = 0
            continue
        h = uc.untril(np.asarray(seq["pose_info"], np.float32)[i]).astype(dtype)
        c = np.asarray(seq["pivot"], dtype)[i]
        if not (np.isfinite(h).all() and np.isfinite(c).all()):
            refused = True
            continue
        if not h.any():
            f[i] = 0
            continue
        a[i] = x[i] - c
        bi = np.eye(26, dtype=dtype) if "repivot" in drop else bmat(a[i], inverse=True)
        hp[i] = dtype(f[i]) * (bi.T @ h @ bi)
    d = np.zeros((max(n - 1, 0), 26), dtype)
    if not refused:
        for i in range(n - 1):
            d[i, :20] = wrap(ja[i + 1, :20] - ja[i, :20])
            d[i, 20:23] = so3_log(rot[i + 1] @ rot[i].T)
            d[i, 23:] = x[i + 1] - x[i]
    if "sign" in drop:
        d = -d
    return dict(x=x, a=a, hp=hp, d=d, w=w32.astype(dtype), f=f, refused=bool(refused))


def pivot_rule(m):
    """(smallest scaled pivot, regular) of a 26 x 26 matrix under uc.scaled_factor's rule, in the matrix's dtype."""
    _low, _sd, least, alive = uc.scaled_factor(m[None])
    return least[0], bool(alive[0])


def dense(p):
    """The float64 dense solve: (u [T,26], C [T,26,26], regular).  Regular: the pivot rule on the last frame's filtered P, which
    the float64 recursion supplies - the dense matrix is singular exactly when that one is."""
    hp, d, w = p["hp"].astype(np.float64), p["d"].astype(np.float64), np.diag(p["w"].astype(np.float64))
    n = len(hp)
    a, g = np.zeros((26 * n, 26 * n)), np.zeros(26 * n)
    for t in range(n):
        a[26 * t:26 * t + 26, 26 * t:26 * t + 26] += hp[t]
    for t in range(n - 1):
        i, j = slice(26 * t, 26 * t + 26), slice(26 * t + 26, 26 * t + 52)
        a[i, i] += w
        a[j, j] += w
        a[i, j] -= w
        a[j, i] -= w
        g[i] += w @ d[t]                                 # d/du of (d + u_j - u_i)^T W (...): -W(...) at i, +W(...) at j
        g[j] -= w @ d[t]
    rec = recursion(p, np.float64, "lu")
    if not rec["regular"]:
        return np.zeros((n, 26)), np.full((n, 26, 26), np.inf), False
    s = 1 / np.sqrt(np.diag(a))                          # Jacobi scaling: the angles' and the translation's entries differ by 1e6
    inv = np.linalg.inv(a * s[:, None] * s[None, :]) * s[:, None] * s[None, :]
    u = (inv @ g).reshape(n, 26)
    c = np.stack([inv[26 * t:26 * t + 26, 26 * t:26 * t + 26] for t in range(n)])
    return u, c, True


def _solver(s, dtype, method):
    """x -> S^-1 x in dtype: numpy's LU, or the scaled Cholesky factor and two substitutions."""
    if method == "lu":
        return lambda rhs: np.linalg.solve(s, rhs).astype(dtype)
    assert method == "cholesky", method
    low, sd, _least, _alive = uc.scaled_factor(s[None])
    fac = (low[0] * sd[0][:, None]).astype(dtype)

    def solve(rhs):
        cols = rhs.reshape(26, -1).astype(dtype)
        y = uc.forward_substitution(fac[None], cols[None])[0]
        x = np.zeros_like(y)
        for i in range(25, -1, -1):
            x[i] = (y[i] - fac[i + 1:, i] @ x[i + 1:]) / fac[i, i]
        return x.astype(dtype).reshape(rhs.shape)
    return solve


def recursion(p, dtype=np.float64, method="lu", product=True):
    """The header's recursion in dtype: dict(u [T,26], c [T,26,26], pivot [T], regular)."""
    hp, d, wv = p["hp"].astype(dtype), p["d"].astype(dtype), p["w"].astype(dtype)
    n = len(hp)
    w = np.diag(wv)
    eye = np.eye(26, dtype=dtype)
    pm, eta = hp[0].copy(), np.zeros(26, dtype)
    keep, pivots = [], np.zeros(n, dtype)
    with np.errstate(all="ignore"):
        for t in range(1, n):
            s = (pm + w).astype(dtype)
            pivots[t - 1] = pivot_rule(s)[0]
            solve = _solver(s, dtype, method)
            keep.append((solve, eta.copy()))
            if product:
                m = (wv[:, None] * solve(pm)).astype(dtype)
            else:
                m = (w - w @ solve(w)).astype(dtype)
            eta = (wv * solve(eta - pm @ d[t - 1])).astype(dtype)
            pm = (dtype(0.5) * (m + m.T) + hp[t]).astype(dtype)
        pivots[n - 1], regular = pivot_rule(pm)
        if not regular:
            return dict(u=np.zeros((n, 26), dtype), c=np.full((n, 26, 26), np.inf, dtype), pivot=pivots, regular=False)
        solve = _solver(pm, dtype, method)
        u, c = np.zeros((n, 26), dtype), np.zeros((n, 26, 26), dtype)
        u[n - 1], c[n - 1] = solve(eta), solve(eye)
        for t in range(n - 2, -1, -1):
            solve, eta_t = keep[t]
            u[t] = solve(eta_t + wv * (u[t + 1] + d[t]))
            g = (solve(eye) * wv[None, :]).astype(dtype)                      # S^-1 W
            c[t] = (solve(eye) + g @ c[t + 1] @ g.T).astype(dtype)
    return dict(u=u, c=c, pivot=pivots, regular=True)


def smooth(seq, dtype=np.float64, method="dense", product=True, drop=()):
    """ut_smooth_pose_sequence on one sequence: dict(ja [T,22], xf [T,4,4], sigma [T,26], info [T,4], u [T,26]) in dtype.  method
    "dense": the float64 oracle."""
    ja, xf = np.asarray(seq["ja"], np.float32), np.asarray(seq["xf"], np.float32)
    n = len(ja)
    out = dict(ja=ja.astype(dtype), xf=xf.astype(dtype), sigma=np.zeros((n, 26), dtype), info=np.zeros((n, 4), dtype), u=np.zeros((n, 26), dtype))
    out["xf"][:, 3] = (0, 0, 0, 1)
    p = prepare(seq, np.float64 if method == "dense" else dtype, drop)
    if p["refused"]:
        out["info"][:, 3] = REFUSED
        return out
    if method == "dense":
        assert dtype == np.float64
        u, c, regular = dense(p)
        pivots = recursion(p, np.float64, "lu")["pivot"]
    else:
        r = recursion(p, dtype, method, product)
        u, c, regular, pivots = r["u"], r["c"], r["regular"], r["pivot"]
    out["info"][:, 2] = pivots
    if not regular:
        out["sigma"][:] = np.inf
        out["info"][:, 3] = SINGULAR
        return out
    ts = dtype(seq["t_scale"])
    wv = p["w"].astype(dtype)
    with np.errstate(all="ignore"):
        for t in range(n):
            delta = bmat(p["a"][t].astype(dtype), inverse=True) @ u[t]
            out["ja"][t, :20] = wrap(out["ja"][t, :20] + delta[:20])
            e = so3_exp(delta[20:23])
            c0 = (p["x"][t] - p["a"][t]).astype(dtype)
            rot, tr = out["xf"][t, :3, :3].copy(), out["xf"][t, :3, 3] * ts
            out["xf"][t, :3, :3] = e @ rot
            out["xf"][t, :3, 3] = (e @ (tr - c0) + c0 + delta[23:]) / ts
            out["sigma"][t] = np.sqrt(np.diagonal(c[t]))
            m = p["d"][t].astype(dtype) + u[t + 1] - u[t] if t < n - 1 else np.zeros(26, dtype)
            out["info"][t, 0] = np.sqrt(max(u[t] @ p["hp"][t].astype(dtype) @ u[t], 0))
            out["info"][t, 1] = np.sqrt((wv * m * m).sum())
            out["info"][t, 3] = OK | (0 if p["f"][t] > 0 else GAP)
    out["u"] = np.asarray(u, dtype)
    return out


# ----------------------------------------------------------------------------- distances and bounds
def landmarks(seq, res):
    m = fc.effective_wrist(np.asarray(res["xf"], np.float64), seq["mirror"], seq["t_scale"], np.float64)
    return fc.forward(seq["hm"], np.asarray(res["ja"], np.float64)[:, :20], m, np.float64)


def distance(seq, got, want):
    """How far a result lies from `want`.  ang, kp: st.distance's (20 angles modulo 2 pi and the wrist's rotation entries in rad;
    landmarks through the float64 forward function in mm).  sigma: param_sigma relative.  moved, stepped: info[0] and info[1]
    absolute, in sigmas.  pivot: info[2] absolute.  Statuses must agree: inf otherwise."""
    sg, sw = np.asarray(got["info"], np.float64)[:, 3], np.asarray(want["info"], np.float64)[:, 3]
    ig, iw = np.asarray(got["info"], np.float64), np.asarray(want["info"], np.float64)
    out = dict(ang=st.angle_and_rotation_distance(got, want), kp=float(np.linalg.norm(landmarks(seq, got) - landmarks(seq, want), axis=-1).max()))
    fin = np.isfinite(np.asarray(want["sigma"], np.float64)) & (np.asarray(want["sigma"], np.float64) > 0)
    gs, ws = np.asarray(got["sigma"], np.float64), np.asarray(want["sigma"], np.float64)
    with np.errstate(all="ignore"):
        rel = np.where(fin, np.abs(gs - ws) / np.where(fin, ws, 1), np.where(gs == ws, 0.0, np.inf))
    out.update(sigma=float(rel.max()), moved=float(np.abs(ig[:, 0] - iw[:, 0]).max()), stepped=float(np.abs(ig[:, 1] - iw[:, 1]).max()),
               pivot=float(np.abs(ig[:, 2] - iw[:, 2]).max()))
    if not np.array_equal(sg, sw):
        out = {k: np.inf for k in out}
    return {k: (v if np.isfinite(v) else np.inf) for k, v in out.items()}


def float32_distance(seq, want=None):
    """The worst distance of the float32 restatements (st.SOLVERS' solves) from the float64 oracle on a sequence."""
    want = smooth(seq) if want is None else want
    return st.worst([distance(seq, smooth(seq, np.float32, s), want) for s in st.SOLVERS])


def bounds_from(d32):
    """DESIGN's rule: the project's bounds, or st.FLOAT32_FACTOR x the float32 restatements' own distance where that is more.
    sigma, moved and stepped have no project bound; their floor is the factor x 26 x 2^-24 x 1e2: 26 roundings of a row at the scaled
    condition 1e2 and below that the unit-diagonal matrices keep (relative for sigma; moved and stepped are of order 1).  The pivot:
    the factor x 26 x 2^-24, as uncertainty_cases.bounds_from."""
    f = st.FLOAT32_FACTOR
    floor = f * 26 * 2.0 ** -24
    return dict(ang=max(st.ANGLE_TOL_RAD, f * d32["ang"]), kp=max(st.KP_TOL_MM, f * d32["kp"]), sigma=max(100 * floor, f * d32["sigma"]),
                moved=max(100 * floor, f * d32["moved"]), stepped=max(100 * floor, f * d32["stepped"]), pivot=max(floor, f * d32["pivot"]))


within = st.within


# ----------------------------------------------------------------------------- sequences of recording_00
@functools.lru_cache(maxsize=None)
def _labels():
    from absolutetrack_amd import pipeline
    lab = pipeline.load_labels()
    ja, xf, hand = mc.label_poses(lab)
    return lab, ja, xf, hand, mc.skeleton(np.load(pipeline._DATA), "hm.")


def centre_of(hm, hand):
    """The default centre of hand.smooth_poses: the mean of the landmarks' rest positions, x negated for a mirrored hand."""
    b = np.asarray(hm["landmark_rest_positions"], np.float64).mean(0)
    if hand == 1:
        b[0] = -b[0]
    return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def recording(first, last, hand, views, noise, seed=None):
    """Frames first..last of recording_00, one hand: the label poses -> their exact windows in the `views` cameras that see most
    landmarks of the frame + Gaussian noise of `noise` px (seed 5 + hand) -> vc.fit_views, every frame started from its label
    -> uc.information at the fits with weights 1 / noise^2.  Returns the sequence, with
    truth_ja / truth_xf the labels and `views_case` what uc.information read.  Cached: leave it unchanged."""
    from absolutetrack_amd import geometry
    lab, lja, lxf, _hand, hm = _labels()
    frames = np.arange(first, last + 1)
    n, cams = len(frames), lab["cameras"]
    n_cam = cams.shape[0]
    idx = 2 * frames + hand
    tja, txf = lja[idx].astype(np.float64), lxf[idx].astype(np.float64)
    mirror = np.full(n, hand, np.int64)
    table = np.stack([geometry.pack_source_camera(cams[ci, 2:4], cams[ci, 4:6], cams[ci, 6:14], lab["camera_to_world_transforms"][f, ci])
                      for f in frames for ci in range(n_cam)])
    truth = fc.forward(hm, tja[:, :20], fc.effective_wrist(txf, mirror, 1.0, np.float64))
    rows_all = (np.arange(n)[:, None] * n_cam + np.arange(n_cam)[None]).astype(np.int32)
    win_all = vc.exact_windows(table, rows_all, truth)
    kind = tc.FISHEYE62
    z = np.stack([tc.project(table[rows_all[:, v], None, :], truth, kind)[1] for v in range(n_cam)], 1)
    wid, hgt = int(cams[0, 0]), int(cams[0, 1])
    seen = (z > 0) & (win_all >= 0).all(-1) & (win_all[..., 0] < wid) & (win_all[..., 1] < hgt)
    order = np.argsort(-seen.sum(2), axis=1, kind="stable")[:, :views]
    cols = np.sort(order, 1)
    rng = np.random.default_rng(5 + hand if seed is None else seed)
    window = np.take_along_axis(win_all, cols[:, :, None, None], 1) + rng.normal(0.0, noise, (n, views, 21, 2))
    cam_rows = np.take_along_axis(rows_all, cols, 1).astype(np.int32)
    weights = (np.take_along_axis(seen, cols[:, :, None], 1) / noise ** 2).astype(np.float32)
    # every fit starts at its frame's label, as in the trial behind the figures: started from the previous frame's fit, hand 1 of
    # frames 200..263 leaves its basin once and stays out (rms 11.9 mm instead of 1.56), which is the tracker's business, not this test's
    ja, xf, _info, _res = vc.fit_views(hm, window, cam_rows, table, weights, (tja.astype(np.float32), txf.astype(np.float32)), mirror)
    ja, xf = np.asarray(ja, np.float32), np.asarray(xf, np.float32)                      # what a fit's outputs hold
    case = dict(hm=hm, window=window, cam_rows=cam_rows, table=table, weights=weights, mirror=mirror, t_scale=1.0, ja=ja, xf=xf,
                loss="squared", loss_scale=3.0, angle_sigma=None)
    info = uc.information(case)
    centre = centre_of(hm, hand)
    q = step_var().astype(np.float64)                    # one frame has no step of its own
    if n > 1:
        turn = np.stack([so3_log(txf[t + 1, :3, :3] @ txf[t, :3, :3].T) for t in range(n - 1)])
        body = np.einsum("tij,j->ti", txf[:, :3, :3], centre.astype(np.float64)) + txf[:, :3, 3]      # the stored wrist is the proper one
        q = np.concatenate([np.full(20, (wrap(tja[1:, :20] - tja[:-1, :20]) ** 2).mean()), np.full(3, (turn ** 2).mean()),
                            np.full(3, ((body[1:] - body[:-1]) ** 2).mean())])
    return dict(ja=ja, xf=xf, pose_info=uc.tril(info["pose_info"]).astype(np.float32), pivot=info["pivot"].astype(np.float32), weight=None,
                centre=centre, step_var=q.astype(np.float32), t_scale=1.0, hm=hm, mirror=mirror, truth_ja=tja.astype(np.float32),
                truth_xf=txf.astype(np.float32), cov_status=info["info"][:, 3].astype(np.int64), views_case=case)


def cut(seq, sel, **change):
    """Frames `sel` (a slice) of a sequence, with changed fields."""
    out = dict(seq)
    for k in ("ja", "xf", "pose_info", "pivot", "mirror", "truth_ja", "truth_xf", "cov_status"):
        if k in seq:
            out[k] = np.array(seq[k][sel], copy=True)
    if seq.get("weight") is not None:
        out["weight"] = np.array(seq["weight"][sel], copy=True)
    out.pop("views_case", None)
    out.update(change)
    return out


def scaled(seq, factor):
    return dict(seq, step_var=(np.asarray(seq["step_var"], np.float64) * factor).astype(np.float32))


def rms_to_truth(seq, res):
    """(rms, max) over frames and landmarks of the distance between the result's landmarks and the labels', mm."""
    d = np.linalg.norm(landmarks(seq, res) - landmarks(seq, dict(ja=seq["truth_ja"], xf=seq["truth_xf"])), axis=-1)
    return float(np.sqrt((d * d).mean())), float(d.max())


@functools.lru_cache(maxsize=None)
def base():
    """The sequence most tests cut from: frames 200..211, hand 0, two views, 0.5 px."""
    return recording(200, 211, 0, 2, 0.5)


@functools.lru_cache(maxsize=None)
def case(name):
    """Named 12-frame sequences on base().  plain; gaps: weight 0 at the first, a middle and the last frame; rank: frame 5 keeps a
    rank-1 H; centre0: centre None; metres: translations in metres (t_scale 1000); free: the index finger's four angles are observed
    by no frame (rows and columns 4..7 of every H zeroed) - SINGULAR; freed: the same, but frame 6 keeps its H.  Cached."""
    b = cut(base(), slice(0, 12))
    if name == "plain":
        return b
    if name == "gaps":
        w = np.ones(12, np.float32)
        w[[0, 5, 11]] = 0
        w[3] = 2.5
        return dict(b, weight=w)
    if name == "rank":
        h = uc.untril(b["pose_info"])
        v = np.linspace(1.0, 2.0, 26) * np.sqrt(np.diagonal(h[5]))
        h[5] = np.outer(v, v) / 26
        return dict(b, pose_info=uc.tril(h).astype(np.float32))
    if name == "centre0":
        return dict(b, centre=None)
    if name == "metres":
        xf = b["xf"].astype(np.float64)
        xf[:, :3, 3] /= 1000.0
        txf = b["truth_xf"].astype(np.float64)
        txf[:, :3, 3] /= 1000.0
        return dict(b, xf=xf.astype(np.float32), truth_xf=txf.astype(np.float32), t_scale=1000.0)
    if name in ("free", "freed"):
        h = uc.untril(b["pose_info"])
        keep = h[6].copy()
        h[:, 4:8, :] = 0
        h[:, :, 4:8] = 0
        if name == "freed":
            h[6] = keep
        return dict(b, pose_info=uc.tril(h).astype(np.float32))
    raise KeyError(name)


CASES = ("plain", "gaps", "rank", "centre0", "metres")
