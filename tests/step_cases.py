"""Shared by tests/test_step_host.py and tests/test_gpu_fit_step.py: cases that pin ONE step of the pose fits' solver
(csrc/ut_fit_dev.h: fit_pose under ut_fit_pose, ut_fit_pose_scale and ut_fit_pose_info) instead of the end of a fit.

A damped solver forgives a wrong Jacobian - it still converges, in more iterations - so the end-to-end tests cannot see one.
One step can: a warm start with max_iters = 1 returns start (+) delta, and the float64 restatements fit_cases.fit,
scale_cases.fit_scale and info_cases.fit_info return the same thing from the same inputs.  The yardstick is those
restatements in float64; the same code in float32 - with numpy's LU solve and with a Cholesky solve, the worst of the two -
says what float32 can give and sets the tolerances (tolerance(), bounds_from()).

Skinning tables.  The stock model binds 20 of 21 landmarks to one frame, so the sparse Jacobian of fit_linearise runs on one
blended landmark only.  TABLE_A and TABLE_B replace rows of landmark_rest_bone_weights / _indices (frames: 0, 1 the wrist,
2 + 3 c + m - 1 the frame after joints 0 .. m of finger c); "mixed" is one model row per pose, rows cycling A, B, stock, so
a wrong model-row index shows.  The dense weights (the last non-zero entry naming a frame wins, mesh_cases.
dense_landmark_weights) of every landmark must sum to 1: the wrist columns of both Jacobians - the restatement's and the
kernel's - are those of the blended landmark as a whole and assume it.  blend() asserts that.

Every case is a dict: hm (the five skinning fields, unbatched or one row per pose), targets (float32, the float64 forward
function of the label poses on that skeleton), mirror, init (float32 start), t_scale, and per entry weights / factors /
init_scale / mode / limits.  The restatements and the kernel see the same float32 numbers."""
import contextlib
import functools

import numpy as np

import fit_cases as fc
import info_cases as ic
import mesh_cases as mc
import scale_cases as sc
from absolutetrack_amd import pipeline

KP_TOL_MM, ANGLE_TOL_RAD = 1e-3, 1e-4     # the project's bounds (tests/test_gpu_fit.py)
SCALE_TOL = 1e-5                          # KP_TOL_MM over the ~100 mm a fingertip lies from the wrist: the scale error that
                                          # moves a landmark by the landmark bound
FLOAT32_FACTOR = 4.0                      # kernel vs numpy's float32 at equal conditioning: Cholesky for LU, FMA, butterflies
N = 24
CLAMP = 0.01                              # so3_exp_map's clamp in rad: the analytic Jacobian deliberately ignores it
FIELDS = sc._FIELDS

# landmark: (weights, indices)
TABLE_A = {
    0: ((0.5, 0.3, 0.2), (4, 3, 2)),            # three frames of one chain, descending
    1: ((0.25, 0.75, 0.0), (5, 7, 7)),          # a zero-weight entry naming a live frame
    2: ((0.7, 0.625, 0.375), (10, 9, 10)),      # first entry dead: frame 10 gets 0.375
    3: ((0.4, 0.35, 0.25), (13, 10, 1)),        # two fingers and the wrist
    4: ((0.0, 0.0, 1.0), (0, 2, 16)),           # the live entry last, dead ones naming other frames
    9: ((0.6, 0.4, 0.0), (5, 0, 3)),            # wrist slot 0
    20: ((0.5, 0.25, 0.25), (1, 11, 5)),        # wrist slot 1 first, then unsorted
}
TABLE_B = {
    0: ((0.5, 0.5, 0.0), (3, 4, 2)),            # two frames ascending, the zero entry naming a frame of the same chain
    1: ((0.75, 0.25, 0.0), (7, 1, 7)),          # a zero-weight entry AFTER the live one naming its frame: it must not kill it
    4: ((0.25, 0.25, 0.5), (16, 15, 14)),       # a whole chain, descending, the proximal frame heaviest
    6: ((0.9, 0.5, 0.5), (2, 2, 6)),            # first entry killed by its neighbour; thumb and index
    10: ((0.5, 0.5, 0.0), (0, 1, 9)),           # both wrist slots and nothing else: no joint column at all
    13: ((0.125, 0.375, 0.5), (16, 4, 9)),      # three fingers
    16: ((0.3, 0.6, 1.0), (12, 12, 12)),        # two dead entries, one frame
    20: ((0.5, 0.5, 0.0), (14, 8, 1)),          # the palm on two proximal frames, no wrist
}
TABLES = ("stock", "a", "b", "mixed")
ENTRIES = ("fit", "scale_free", "scale_fixed", "info")


# ----------------------------------------------------------------------------- skeletons
@functools.lru_cache(maxsize=None)
def _stock():
    return mc.skeleton(np.load(pipeline._DATA), "hm.")


def joint_limits():
    return _stock()["joint_limits"][:20].astype(np.float32)


def blend(rows):
    """The stock skeleton with the landmark rows of `rows` replaced."""
    hm = {k: np.array(_stock()[k]) for k in FIELDS}
    for lm, (w, idx) in rows.items():
        assert min(idx) >= 0 and max(idx) <= 16
        hm["landmark_rest_bone_weights"][lm] = w
        hm["landmark_rest_bone_indices"][lm] = idx
    total = mc.dense_landmark_weights(hm).astype(np.float64).sum(1)
    assert np.abs(total - 1).max() <= 1e-6, total                 # the wrist columns of the Jacobians assume it
    return hm


def _single(table):
    return blend({"stock": {}, "a": TABLE_A, "b": TABLE_B}[table])


def skeleton(table, n=N):
    """'stock', 'a', 'b': one model; 'mixed': n rows cycling a, b, stock."""
    if table != "mixed":
        return _single(table)
    rows = [_single(("a", "b", "stock")[i % 3]) for i in range(n)]
    return {k: np.stack([r[k] for r in rows]) for k in FIELDS}


def rows_of(hm, sel):
    return fc._take(hm, np.asarray(sel))


# ----------------------------------------------------------------------------- poses and starts
@functools.lru_cache(maxsize=None)
def labels():
    ja, xf, hand = mc.label_poses(pipeline.load_labels())
    return ja, xf, hand


def perturbed(ja, xf, seed, angle, rotation, shift):
    """Labels plus uniform noise (rad on the 20 angles, rad on the wrist's rotation vector, mm), rounded to float32."""
    rng = np.random.default_rng(seed)
    ja0 = ja.copy()
    ja0[:, :20] += rng.uniform(-angle, angle, (len(ja), 20))
    xf0 = xf.copy()
    xf0[:, :3, :3] = fc._rodrigues(rng.uniform(-rotation, rotation, (len(ja), 3))) @ xf0[:, :3, :3]
    xf0[:, :3, 3] += rng.uniform(-shift, shift, (len(ja), 3))
    return ja0.astype(np.float32), xf0.astype(np.float32)


@functools.lru_cache(maxsize=None)
def poses():
    """24 label poses of recording_00, hands alternating (pose i is hand i % 2, right ones through `mirror`), and their
    starts: +-0.2 rad, +-0.2 rad, +-15 mm (seed 31).  No label angle and no start angle lies inside so3_exp_map's clamp."""
    ja, xf, hand = labels()
    ja0, xf0 = perturbed(ja, xf, 31, 0.2, 0.2, 15.0)
    ok = (np.abs(ja[:, :20]) >= CLAMP).all(1) & (np.abs(ja0[:, :20]) >= CLAMP).all(1)
    sel = np.zeros(N, np.int64)
    for h in range(2):
        cand = np.nonzero(ok & (hand == h))[0]
        assert len(cand) >= N // 2, (h, len(cand))
        sel[h::2] = cand[np.linspace(0, len(cand) - 1, N // 2).astype(np.int64)]
    assert len(set(sel)) == N
    return dict(sel=sel, ja=ja[sel], xf=xf[sel], hand=hand[sel], ja0=ja0[sel], xf0=xf0[sel])


def label_targets(hm, ja, xf, hand):
    """The float64 forward function of label poses on `hm`, rounded to float32."""
    return fc.forward(hm, ja, fc.effective_wrist(xf, hand, 1.0, np.float64)).astype(np.float32)


def _weights(group, n):
    rng = np.random.default_rng(47)
    w = np.ones((n, 21), np.float32)
    if group == "hidden":
        w[np.arange(n), rng.integers(0, 21, n)] = 0
    elif group == "spread":
        w = (10.0 ** rng.uniform(-1, 1, (n, 21))).astype(np.float32)
    return w


def _factors(group, n):
    """'unit': the identity.  'aniso': lower Cholesky factors of R diag(1, 10^-u, 10^-v)^2 R^T, R a random rotation, u in
    [0, 1], v in [0, 2] - axis ratios down to 1:100 - and one landmark per pose all zero."""
    if group != "aniso":
        return ic.isotropic(np.ones((n, 21), np.float32))
    rng = np.random.default_rng(53)
    r = fc._rodrigues(rng.uniform(-np.pi, np.pi, (n * 21, 3)) / np.sqrt(3))
    d = np.stack([np.ones(n * 21), 10.0 ** -rng.uniform(0, 1, n * 21), 10.0 ** -rng.uniform(0, 2, n * 21)], 1)
    low = np.linalg.cholesky(r @ (d[:, :, None] ** 2 * r.transpose(0, 2, 1)))
    f = np.stack([low[:, 0, 0], low[:, 1, 0], low[:, 1, 1], low[:, 2, 0], low[:, 2, 1], low[:, 2, 2]], 1).reshape(n, 21, 6)
    f[np.arange(n), rng.integers(0, 21, n)] = 0
    return f.astype(np.float32)


def groups(entry, table):
    """The weight groups of a table: unit, one landmark at 0, spread 10^+-1 (info: unit and anisotropic factors); on the
    mixed table also 'metres': unit weights, t_scale = 1000, and the GPU test hands the wrist out with xf_stride = 12."""
    g = ("unit", "aniso") if entry == "info" else ("unit", "hidden", "spread")
    return g + (("metres",) if table == "mixed" else ())


def all_cases():
    return [(e, t, g) for e in ENTRIES for t in TABLES for g in groups(e, t)]


def _entry_fields(entry, group, n):
    c = dict(weights=None, factors=None, init_scale=None, mode=sc.FREE, limits=None)
    if entry == "info":
        c["factors"] = _factors(group, n)
    else:
        c["weights"] = _weights(group, n)
    if entry.startswith("scale"):
        c["init_scale"] = np.where(np.arange(n) % 4 < 2, 0.9, 1.1).astype(np.float32)      # away from the targets' 1
        c["mode"] = sc.FIXED if entry == "scale_fixed" else sc.FREE
    return c


@functools.lru_cache(maxsize=None)
def case(entry, table, group):
    """The one-step case of (entry, table, group) on the 24 poses.  Cached: leave it unchanged."""
    p = poses()
    hm = skeleton(table)
    t_scale = 1000.0 if group == "metres" else 1.0
    xf0 = p["xf0"].copy()
    xf0[:, :3, 3] = (xf0[:, :3, 3].astype(np.float64) / t_scale).astype(np.float32)
    c = dict(entry=entry, hm=hm, targets=label_targets(hm, p["ja"], p["xf"], p["hand"]), mirror=p["hand"], init=(p["ja0"], xf0),
             t_scale=t_scale)
    c.update(_entry_fields(entry, group, N))
    return c


def subset(c, sel):
    """Poses `sel` of a case, the model rows with them when there is one per pose."""
    sel = np.asarray(sel)
    out = dict(c, hm=rows_of(c["hm"], sel), targets=c["targets"][sel], mirror=c["mirror"][sel],
               init=(c["init"][0][sel], c["init"][1][sel]))
    for k in ("weights", "factors", "init_scale"):
        out[k] = None if c[k] is None else c[k][sel]
    if c["limits"] is not None and np.asarray(c["limits"]).ndim == 3:
        out["limits"] = c["limits"][sel]
    return out


# ----------------------------------------------------------------------------- the restatements
SOLVERS = ("lu", "cholesky")


def cholesky_solve(a, b):
    """fc.solve by a Cholesky factorisation and two substitutions, in the dtype of `a`: the kernel's algorithm, where numpy's
    solve is LU with pivoting."""
    low = np.linalg.cholesky(a)
    vec = b.ndim == a.ndim - 1
    rhs = b[..., None] if vec else b
    n = a.shape[-1]
    y = np.zeros_like(rhs)
    for i in range(n):
        y[..., i, :] = (rhs[..., i, :] - np.einsum("...j,...jk->...k", low[..., i, :i], y[..., :i, :])) / low[..., i, i, None]
    x = np.zeros_like(rhs)
    for i in range(n - 1, -1, -1):
        x[..., i, :] = (y[..., i, :] - np.einsum("...j,...jk->...k", low[..., i + 1:, i], x[..., i + 1:, :])) / low[..., i, i, None]
    return x[..., 0] if vec else x


@contextlib.contextmanager
def solver(name):
    """The restatements with fc.solve = numpy's LU ('lu', as they stand) or cholesky_solve."""
    keep = fc.solve
    try:
        if name == "cholesky":
            fc.solve = cholesky_solve
        else:
            assert name == "lu", name
        yield
    finally:
        fc.solve = keep


def restate(c, dtype=np.float64, max_iters=1, trace=None, solve="lu"):
    """k iterations of the case's restatement from its start: dict(ja [n,22], xf [n,4,4], scale [n], info [n,4 or 6])."""
    with solver(solve):
        return _restate(c, dtype, max_iters, trace)


def _restate(c, dtype, max_iters, trace):
    kw = dict(limits=c["limits"], init=c["init"], mirror=c["mirror"], t_scale=c["t_scale"], max_iters=max_iters, dtype=dtype,
              trace=trace)
    if c["entry"] == "fit":
        ja, xf, info = fc.fit(c["hm"], c["targets"], weights=c["weights"], **kw)
    elif c["entry"] == "info":
        ja, xf, info = ic.fit_info(c["hm"], c["targets"], c["factors"], **kw)
    else:
        ja, xf, s, info = sc.fit_scale(c["hm"], c["targets"], weights=c["weights"], init_scale=c["init_scale"], mode=c["mode"], **kw)
        return dict(ja=ja, xf=xf, scale=s, info=info)
    return dict(ja=ja, xf=xf, scale=np.ones(len(ja), dtype), info=info)


@functools.lru_cache(maxsize=None)
def step(entry, table, group, dtype=np.float64, max_iters=1, solve="lu"):
    """(result, trace) of the restatement on case(entry, table, group).  Cached: leave it unchanged."""
    trace = []
    return restate(case(entry, table, group), dtype, max_iters, trace, solve), trace


def landmarks(c, res):
    """The float64 forward function of a result on the case's skeleton, at the result's scale."""
    m = fc.effective_wrist(np.asarray(res["xf"], np.float64), c["mirror"], c["t_scale"], np.float64)
    return sc.forward(c["hm"], np.asarray(res["scale"], np.float64), np.asarray(res["ja"], np.float64)[:, :20], m, np.float64)


def angle_and_rotation_distance(a, b):
    """The `ang` of distance(), here and in views_cases: the 20 angles modulo 2 pi and the entries of the wrist's rotation, rad."""
    return float(max(fc.angle_distance(a["ja"][:, :20], b["ja"][:, :20]).max(),
                     np.abs(np.asarray(a["xf"], np.float64)[:, :3, :3] - np.asarray(b["xf"], np.float64)[:, :3, :3]).max()))


def distance(c, a, b):
    """How far two results of a case lie apart.  ang: the 20 angles modulo 2 pi and the entries of the wrist's rotation, rad.
    kp: landmarks through the float64 forward function of both (which carries the wrist's translation), and rms / worst of
    info, mm.  scale: |s_a - s_b|.  scale_info: info[4] relative to b's (0 where the entry has none)."""
    ia, ib = np.asarray(a["info"], np.float64), np.asarray(b["info"], np.float64)
    kp = max(np.linalg.norm(landmarks(c, a) - landmarks(c, b), axis=-1).max(), np.abs(ia[:, :2] - ib[:, :2]).max())
    out = dict(ang=angle_and_rotation_distance(a, b), kp=float(kp), scale=float(np.abs(np.asarray(a["scale"], np.float64) - b["scale"]).max()),
               scale_info=0.0)
    if c["entry"] == "scale_free":
        out["scale_info"] = float((np.abs(ia[:, 4] - ib[:, 4]) / ib[:, 4]).max())
    return out


def bounds_from(d32):
    """The GPU bounds of a case from the distance between its float32 and float64 restatements: the project's bounds where
    float32 stays within a quarter of them, else FLOAT32_FACTOR x that distance.  The scale information has no project
    bound: always the factor.  The float32 distance is the worst of two float32 restatements that differ in the linear
    solve alone (SOLVERS): the worst pose of a group is an ill-conditioned one, where one float32 run is one draw of the
    rounding - with a fingertip hidden on TABLE_B the Cholesky run lies 9.4e-4 mm from float64 and the LU run 2.9e-4 mm."""
    return dict(ang=max(ANGLE_TOL_RAD, FLOAT32_FACTOR * d32["ang"]), kp=max(KP_TOL_MM, FLOAT32_FACTOR * d32["kp"]),
                scale=max(SCALE_TOL, FLOAT32_FACTOR * d32["scale"]), scale_info=FLOAT32_FACTOR * d32["scale_info"])


def worst(distances):
    return {k: max(d[k] for d in distances) for k in distances[0]}


def float32_distance(entry, table, group, max_iters=1):
    """The worst distance of a float32 restatement - one per solver of SOLVERS - from the float64 one on a cached case."""
    c, want = case(entry, table, group), step(entry, table, group, np.float64, max_iters)[0]
    return worst([distance(c, step(entry, table, group, np.float32, max_iters, s)[0], want) for s in SOLVERS])


def float32_distance_of(c, want, max_iters=1):
    """float32_distance for a case that is not one of case(): `want` is its float64 result."""
    return worst([distance(c, restate(c, np.float32, max_iters, solve=s), want) for s in SOLVERS])


def tolerance(entry, table, group):
    """The bounds the GPU's one step is held to on case(entry, table, group): computed from the two restatements, never
    from the kernel."""
    return bounds_from(float32_distance(entry, table, group))


def decisions(res, trace):
    """(first trial accepted, iterations, status) per pose."""
    return trace[0]["accept"].copy(), res["info"][:, 2].astype(np.int64), res["info"][:, 3].astype(np.int64)


def within(d, tol):
    """Every figure of a distance() - this module's or views_cases' - within its bound of the matching bounds_from()."""
    return all(d[k] <= tol[k] for k in d)


# ----------------------------------------------------------------------------- wrong Jacobians, for the sensitivity test
@contextlib.contextmanager
def wrong(defect):
    """The restatements with one defect in the linearisation only - what a wrong kernel would do:
    'stock_table'   the Jacobian of the stock skinning table, whatever the forward function uses
    'first_wins'    dense weights where the first non-zero entry naming a frame wins (the entries reversed)
    'no_mirror'     the joint columns without the sign of the wrist's determinant
    'no_sigma'      the scale's column dropped
    'transposed'    residuals and Jacobian rows whitened by L instead of L^T."""
    fc_jac, sc_jac, ic_whiten = fc.jacobian, sc.jacobian, ic.whiten

    def with_table(hm, b, reverse):
        out = dict(hm)
        for k in ("landmark_rest_bone_weights", "landmark_rest_bone_indices"):
            v = np.asarray(hm[k])[..., ::-1] if reverse else np.asarray(_stock()[k])
            out[k] = v if np.asarray(hm[k]).ndim == 2 else np.broadcast_to(v, np.asarray(hm[k]).shape)
        return out

    def jac(hm, angles, eff_wrist, centroid, dtype=np.float64):
        if defect in ("stock_table", "first_wins"):
            hm = with_table(hm, len(angles), defect == "first_wins")
        j = fc_jac(hm, angles, eff_wrist, centroid, dtype)
        if defect == "no_mirror":
            j[:, :, :20] *= np.sign(np.linalg.det(eff_wrist[:, :3, :3].astype(np.float64))).astype(dtype)[:, None, None]
        return j

    def jac_scale(hm, s, angles, eff_wrist, centroid, dtype=np.float64):
        j = sc_jac(hm, s, angles, eff_wrist, centroid, dtype)
        j[:, :, 26] = 0
        return j

    def whiten_transposed(f, r):
        l = [f[..., k].reshape(f.shape[:2] + (1,) * (r.ndim - 3)) for k in range(6)]
        r0, r1, r2 = r[:, :, 0], r[:, :, 1], r[:, :, 2]
        return np.stack([l[0] * r0, l[1] * r0 + l[2] * r1, l[3] * r0 + l[4] * r1 + l[5] * r2], 2)

    try:
        if defect in ("stock_table", "first_wins", "no_mirror"):
            fc.jacobian = jac
        elif defect == "no_sigma":
            sc.jacobian = jac_scale
        else:
            assert defect == "transposed", defect
            ic.whiten = whiten_transposed
        yield
    finally:
        fc.jacobian, sc.jacobian, ic.whiten = fc_jac, sc_jac, ic_whiten


# ----------------------------------------------------------------------------- starts whose first trial is rejected
RUNS = ((np.float32, "lu"), (np.float32, "cholesky"), (np.float64, "lu"))
REJECT_MARGIN = 1.05      # the first trial's cost is at least this x the start's, in float32 (both solvers) and in float64
ACCEPT_MARGIN = 0.95      # and the second trial's at most this x the start's: neither decision is a close call
REJECT_MAX = 24
REJECT_SCALE = 0.3


@functools.lru_cache(maxsize=None)
def rejected_case(entry):
    """Starts on the stock model whose first trial (lambda = 1e-3) is rejected and whose second (lambda = 1e-2, the same
    linearisation) is accepted: +-1.5 rad on the angles and the wrist's rotation of all 738 label poses, seeds 0 .. 2, kept
    where the float32 and the float64 restatement both decide so with the margins above and every start angle stays inside
    +-3.1 rad (the output wraps beyond pi).  entry: 'fit' or 'scale_free'.  With the scale free and a start scale near the
    targets' (0.9 / 1.1, also 1 and 3.5; noise up to +-3 rad) not one first trial of the 3 x 738 is rejected - shrinking or
    growing the hand always lowers the cost of a wild start - so those starts begin at REJECT_SCALE = 0.3, where the first
    step overshoots the scale.  At most REJECT_MAX poses, in order of seed and pose; later seeds are not searched once there
    are that many.  Returns the case with `found` = (seed, pose) rows and `ratios` [k,3,2] (run of RUNS, trial)."""
    ja, xf, hand = labels()
    hm = skeleton("stock")
    targets = label_targets(hm, ja, xf, hand)
    n = len(ja)
    parts, found, ratios = [], [], []
    for seed in range(3):
        ja0, xf0 = perturbed(ja, xf, seed, 1.5, 1.5, 0.0)
        c = dict(entry=entry, hm=hm, targets=targets, mirror=hand, init=(ja0, xf0), t_scale=1.0)
        c.update(_entry_fields(entry, "unit", n))
        if entry == "scale_free":
            c["init_scale"] = np.full(n, REJECT_SCALE, np.float32)
        keep = np.abs(ja0[:, :20]).max(1) <= 3.1
        ratio = np.zeros((n, 3, 2))
        for k, (dt, how) in enumerate(RUNS):
            trace = []
            restate(c, dt, 2, trace, how)
            first, second = trace
            ratio[first["idx"], k, 0] = first["trial_cost"] / first["cost"]
            later = np.full(n, np.inf)
            later[second["idx"]] = second["trial_cost"] / second["cost"]
            ratio[:, k, 1] = later
            rejected = np.zeros(n, bool)
            rejected[first["idx"]] = ~first["accept"] & (first["trial_cost"] >= REJECT_MARGIN * first["cost"])
            accepted = np.zeros(n, bool)
            accepted[second["idx"]] = second["accept"] & (second["trial_cost"] <= ACCEPT_MARGIN * second["cost"])
            keep &= rejected & accepted
        sel = np.nonzero(keep)[0]
        parts.append(subset(c, sel))
        found += [(seed, int(i)) for i in sel]
        ratios.append(ratio[sel])
        if len(found) >= REJECT_MAX:
            break
    out = dict(parts[0], hm=hm)
    out["targets"], out["mirror"] = (np.concatenate([p[k] for p in parts])[:REJECT_MAX] for k in ("targets", "mirror"))
    out["init"] = tuple(np.concatenate([p["init"][k] for p in parts])[:REJECT_MAX] for k in range(2))
    for k in ("weights", "init_scale"):
        out[k] = None if parts[0][k] is None else np.concatenate([p[k] for p in parts])[:REJECT_MAX]
    out["found"], out["ratios"] = found[:REJECT_MAX], np.concatenate(ratios)[:REJECT_MAX]
    return out


# ----------------------------------------------------------------------------- a hidden finger, a step into the wall
def finger_frames(c):
    return range(2 + 3 * c, 5 + 3 * c)


def observable(hm, weights):
    """[n,20] bool: joint 4 c + j moves a landmark with a positive weight - one carried by a frame after that joint,
    frames m >= max(j, 1) of finger c.  The column of any other joint is zero, and the diagonal's floor keeps it where it is."""
    n = len(weights)
    dense = fc._model(hm, n, np.float64)[3]                                      # [n,21,17]
    seen = ((dense != 0) & (np.asarray(weights) > 0)[..., None]).any(1)          # [n,17]: a visible landmark on the frame
    out = np.zeros((n, 20), bool)
    for c in range(5):
        for j in range(4):
            out[:, 4 * c + j] = seen[:, [2 + 3 * c + m - 1 for m in range(max(j, 1), 4)]].any(1)
    return out


@functools.lru_cache(maxsize=None)
def hidden_case(table):
    """Full fits from the +-0.2 rad starts with landmarks hidden (weight 0).  'stock': pose i hides every landmark that a
    frame of finger i % 5 carries - the palm centre too where the finger is the index or the middle, whose proximal frames
    carry it - so all four joints of that finger are unobservable.  'a': landmark 3 alone, which ties ring and middle: the
    middle finger stays observable through landmarks 2, 12 and 13 and the ring through 15, 16 and the palm, except the ring's
    distal joint, whose frame 13 no other landmark of TABLE_A names.  `seen` = observable()."""
    c = dict(case("fit", table, "unit"))
    w = np.ones((N, 21), np.float32)
    if table == "stock":
        dense = mc.dense_landmark_weights(c["hm"])
        for i in range(N):
            w[i, (dense[:, list(finger_frames(i % 5))] != 0).any(1)] = 0
    else:
        w[:, 3] = 0
    c["weights"] = w
    c["seen"] = observable(c["hm"], w)
    return c


WALL_PUSH = 1e-3      # rad: the unclamped step leaves the box by at least this much
WALL_BEYOND = 0.02    # rad: a label angle this far outside joint_limits pulls its joint into the wall


@functools.lru_cache(maxsize=None)
def wall_case():
    """One step into the box's wall, on the mixed table with one row of joint_limits per model row.  A start on a bound is
    pushed outward when the label lies beyond that bound, so: the 24 label poses (hands alternating) with the most angles
    WALL_BEYOND or more outside joint_limits, at a bound with |bound| >= CLAMP; their +-0.2 rad starts clamped into the
    box; those joints put exactly on that bound.  `wall` [n,20] marks the joints on a bound that the float64 step, before it
    is clamped, pushes outward by WALL_PUSH or more in a pose whose trial the float32 and the float64 restatement both
    accept; `bound` [n,20] float32 is the bound's value."""
    ja, xf, hand = labels()
    ja0, xf0 = perturbed(ja, xf, 31, 0.2, 0.2, 15.0)
    lim = joint_limits()
    lo, hi = lim[:, 0], lim[:, 1]
    below = (ja[:, :20] <= lo - WALL_BEYOND) & (np.abs(lo) >= CLAMP)
    above = (ja[:, :20] >= hi + WALL_BEYOND) & (np.abs(hi) >= CLAMP)
    count = (below | above).sum(1)
    sel = np.zeros(N, np.int64)
    for h in range(2):
        cand = np.nonzero(hand == h)[0]
        sel[h::2] = np.sort(cand[np.argsort(-count[cand], kind="stable")[:N // 2]])
    hm = skeleton("mixed")
    start = np.minimum(np.maximum(ja0[sel], np.concatenate([lo, [-np.inf] * 2]).astype(np.float32)),
                       np.concatenate([hi, [np.inf] * 2]).astype(np.float32))
    at = below[sel] | above[sel]
    bound = np.where(above[sel], hi, np.where(below[sel], lo, 0)).astype(np.float32)
    start[:, :20] = np.where(at, bound, start[:, :20])
    c = dict(entry="fit", hm=hm, targets=label_targets(hm, ja[sel], xf[sel], hand[sel]), mirror=hand[sel], init=(start, xf0[sel]),
             t_scale=1.0)
    c.update(_entry_fields("fit", "unit", N))
    c["limits"] = np.broadcast_to(lim, (N, 20, 2)).copy()
    accepted = np.ones(N, bool)
    for dt, how in RUNS:
        trace = []
        restate(c, dt, 1, trace, how)
        accepted &= trace[0]["accept"]
    delta = trace[0]["delta"][:, :20]
    outward = np.where(above[sel], delta >= WALL_PUSH, delta <= -WALL_PUSH)
    c["wall"], c["bound"] = at & outward & accepted[:, None], bound
    return c


# ----------------------------------------------------------------------------- iterations of full fits
ITERATION_CASES = [(e, t, "aniso" if e == "info" else "unit") for e in ("fit", "scale_free", "info") for t in ("a", "b", "mixed")]


@functools.lru_cache(maxsize=None)
def iteration_yardstick(entry, table, group):
    """Full fits (max_iters = 32) of case(entry, table, group) by the restatements of RUNS, which must converge on every
    pose: (float32 iterations [n], float64 iterations [n], margin, the float32 runs' own counts [2,n]).  A wrong Jacobian
    costs iterations, rounding moves the count by little: the margin is the largest per-pose difference between a float32
    and the float64 count, at least 2, and the kernel - float32 as well - may need the float32 count plus that.  Near the
    end a float32 fit moves at the resolution of its cost, and how many trials that takes is rounding's: the two float32
    runs, which differ in the linear solve alone, are up to 3 (fit) and 9 (info) iterations apart per pose, more than either
    is from float64 on some cases.  So the float32 count is the larger of the two per pose, and the margin is over both."""
    its = []
    for dt, how in RUNS:
        r = restate(case(entry, table, group), dt, 32, solve=how)
        assert np.all(r["info"][:, 3] == fc.CONVERGED), (entry, table, group, dt, how)
        its.append(r["info"][:, 2].astype(np.int64))
    both = np.stack(its[:2])
    return both.max(0), its[2], max(2, int(np.abs(both - its[2]).max())), both
