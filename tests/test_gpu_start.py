"""GPU tests of the start of a pose fit in the views (csrc/start_views.hip through ut_start_pose_views and ut_select_pose,
hand.cold_start_views, hand.fit_landmarks_views_cold) against the float64 restatement of tests/start_cases.py, which
tests/test_start_host.py checks.  Shapes: slices of 1 and 5 of the 74 golden hands, both mirror values; the full chain on all 74.

Bounds (DESIGN.md "One step against float64"): the project's 1e-3 mm on the start's landmarks, or st.FLOAT32_FACTOR x the
distance of the restatement's float32 twin from the float64 restatement on that case, whichever is larger; in px 2^-23 x 300 or
that factor x the twin's distance.  Computed here from the restatements, never from the kernel's output, and printed (-s).  Many
seeds end in the same pose at the same cost, so the winning index is often a tie: every pair is compared by its cost with the
restatement's best, and by its landmarks with the restatement's winner - or, where the restatement's score of the seed the kernel
chose lies within the px bound of its best (either may win), with the restatement's end of that seed on cost alone.  No pair is
left out.  The twin must not leave the float64 restatement's pose (vc.BASIN_MM) on more than 5 % of the pairs."""
import numpy as np
import pytest
import torch

import start_cases as sc
import step_cases as st
import triangulate_cases as tc
import views_cases as vc
from absolutetrack_amd import _native, hand, pipeline, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(*(hm[k] for k in st.FIELDS))).reshape(-1, 321)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hands(n):
    """n golden hands, both mirror values among them when n > 1."""
    m = vc.golden()["hand"]
    left, right = np.flatnonzero(m == 0), np.flatnonzero(m == 1)
    return np.sort(np.concatenate([left[:(n + 1) // 2], right[:n // 2]]))


def _sub(c, sel):
    out = dict(c)
    for k in ("window", "cam_rows", "weights", "mirror", "truth"):
        out[k] = c[k][sel]
    return out


def _case(name):
    """dict(hm, window, cam_rows, table, weights, mirror, limits, t_scale, bank, seeds, xf_stride)."""
    n = 1 if name == "n1_k1_s1_v1" else 5
    c = _sub(sc.golden_case("one" if name == "n1_k1_s1_v1" else "two", 0), _hands(n))
    c.update(bank=sc.bank(), seeds=sc.seeds(), xf_stride=16)
    if name == "n1_k1_s1_v1":
        c.update(bank=sc.bank()[2:3], seeds=sc.seeds()[:1])
    elif name == "ragged_v3":
        c = vc.ragged(c)
    elif name == "pinhole":
        c["table"] = tc.pinhole_from_fisheye(c["table"])
        c["window"] = vc.exact_windows(c["table"], c["cam_rows"], c["truth"])
    elif name == "metres_stride12":
        c.update(t_scale=1000.0, xf_stride=12, limits=st.joint_limits()[None])
    elif name == "three_landmarks":
        w = np.zeros_like(c["weights"])
        for i in range(n):
            seen = np.flatnonzero((c["weights"][i] > 0).all(0))      # one view of three landmarks has up to four poses of cost 0: two views
            w[i, :, seen[[0, len(seen) // 2, -1]]] = 1
        c["weights"] = w
    assert n == 1 or set(c["mirror"]) == {0, 1}
    return c


CASES = ("n1_k1_s1_v1", "n5_k4_s24_v2", "ragged_v3", "pinhole", "metres_stride12", "three_landmarks")


def _restate(c, dtype=np.float64):
    return sc.start_pose_views(c["hm"], c["window"], c["cam_rows"], c["table"], c["bank"], c["seeds"], c["weights"], c["mirror"], c["limits"],
                               c["t_scale"], sc.ITERS, dtype)


def _gpu(c, pad_views=0, engine=None):
    n, v = c["cam_rows"].shape
    win, rows, w = c["window"], c["cam_rows"], c["weights"]
    if pad_views:
        win = np.concatenate([win, np.full((n, pad_views, 21, 2), np.nan)], 1)
        rows = np.concatenate([rows, np.full((n, pad_views), -1, np.int32)], 1)
        w = np.concatenate([w, np.full((n, pad_views, 21), np.nan, np.float32)], 1)
    k = len(c["bank"])
    kw = {}
    guard = None
    if c["xf_stride"] != 16:
        guard = torch.full((n * k + 1, c["xf_stride"]), 7.0, device=DEV)
        kw.update(out=(torch.empty(n * k, 22, device=DEV), guard), xf_stride=c["xf_stride"])
    ja, xf, info = _native.start_pose_views(_blob(c["hm"]), _t(win, torch.float64), _t(rows, torch.int32), _t(c["table"], torch.float64),
                                            _t(c["bank"]), _t(c["seeds"], torch.float64), _t(w), None if c["limits"] is None else _t(c["limits"]),
                                            _t(c["mirror"], torch.int64), c["t_scale"], sc.ITERS, engine=engine, **kw)
    torch.cuda.synchronize()
    xf = xf.cpu().numpy()
    if guard is not None:
        assert np.array_equal(xf[n * k], np.full(c["xf_stride"], 7.0, np.float32))
        xf = np.concatenate([xf[:n * k, :12].reshape(-1, 3, 4), np.tile(np.float32([[[0, 0, 0, 1]]]), (n * k, 1, 1))], 1)
    return dict(ja=ja.cpu().numpy(), xf=xf.reshape(n * k, 4, 4), info=info.cpu().numpy())


def _start_landmarks(c, res):
    k = len(c["bank"])
    r = sc.repeat_case(c, k)
    return vc.landmarks(dict(hm=r["hm"], mirror=r["mirror"], t_scale=c["t_scale"]), res)


# ----------------------------------------------------------------------------- 1. the starts against float64
@pytest.mark.parametrize("name", CASES)
def test_starts_against_float64(name):
    c = _case(name)
    n, k = len(c["mirror"]), len(c["bank"])
    want, twin = _restate(c), _restate(c, np.float32)
    rows = np.arange(n * k)
    ok = want["info"][:, 3] == 0
    assert ok.all() and (twin["info"][:, 3] == 0).all()
    twin_kp = np.linalg.norm(twin["landmarks"] - want["landmarks"], axis=-1).max(1)
    twin_px = np.abs(twin["info"][:, 0].astype(np.float64) - want["info"][:, 0])
    left = twin_kp > vc.BASIN_MM
    assert left.mean() <= 0.05, f"the float32 twin leaves the float64 pose on {left.sum()} of {n * k} pairs: other inputs or more iterations"
    tol_kp = max(st.KP_TOL_MM, sc.FLOAT32_FACTOR * float(twin_kp[~left].max()))
    tol_px = max(300.0 * 2.0 ** -23, sc.FLOAT32_FACTOR * float(twin_px[~left].max()))
    got = _gpu(c)
    assert np.array_equal(got["info"][:, 3], np.zeros(n * k, np.float32))
    assert np.array_equal(_bits(got["ja"]), _bits(want["ja"])) and np.array_equal(got["xf"][:, 3], np.tile(np.float32([0, 0, 0, 1]), (n * k, 1)))
    seed = got["info"][:, 2].astype(np.int64)
    assert np.all((seed >= 0) & (seed < len(c["seeds"])))
    rms_all = want["rms"].reshape(n * k, -1)                                           # every seed's rms in the restatement
    d_px = np.abs(got["info"][:, 0].astype(np.float64) - rms_all.min(1))
    d_kp = np.linalg.norm(_start_landmarks(c, got) - want["landmarks"], axis=-1).max(1)
    either = (rms_all[rows, seed] - rms_all.min(1) <= tol_px) & (seed != want["info"][:, 2])      # the kernel's seed ties with the best
    on_cost_alone = either & (d_kp > tol_kp)
    print(f"{name}: cost {d_px.max():.2e} px (bound {tol_px:.2e}; twin {twin_px.max():.2e}), landmarks {d_kp[~on_cost_alone].max(initial=0):.2e} mm "
          f"(bound {tol_kp:.2e}; twin {twin_kp.max():.2e}); another seed of the same score on {int(either.sum())} of {n * k} pairs, "
          f"{int(on_cost_alone.sum())} of them another pose, compared on cost alone")
    assert d_px.max() <= tol_px, (d_px.max(), tol_px)
    assert np.all((d_kp <= tol_kp) | on_cost_alone), (d_kp.max(), tol_kp)
    assert np.all((seed == want["info"][:, 2]) | either)
    worst = np.abs(got["info"][~on_cost_alone, 1].astype(np.float64) - want["info"][~on_cost_alone, 1])
    assert worst.max(initial=0) <= tol_px + tol_kp * 10.0                              # the golden cameras see under 10 px per mm


# ----------------------------------------------------------------------------- 2. a row alone, in a batch, with padding views
def test_a_row_has_its_bits_alone_in_a_batch_and_with_padding_views():
    c = _case("ragged_v3")
    k = len(c["bank"])
    whole = _gpu(c)
    padded = _gpu(c, pad_views=2)
    assert all(np.array_equal(_bits(whole[f]), _bits(padded[f])) for f in whole)
    for i in (0, 3):
        one = _gpu(_sub(c, np.array([i])))
        assert all(np.array_equal(_bits(one[f]), _bits(whole[f][i * k:(i + 1) * k])) for f in whole), i


# ----------------------------------------------------------------------------- 3. the refusals
def test_refusals_write_what_the_header_says():
    """test_start_host.test_refusals_of_the_restatement's hands on the kernel: the same rows refused with the bank pose at the identity
    and info (0, 0, -1, REFUSED), the others the restatement's; a NaN window at weight 0 changes no bit."""
    c = _sub(sc.golden_case("two", 0), np.arange(6))
    c.update(bank=sc.bank()[:2], seeds=sc.seeds()[:4], xf_stride=16)
    win, w = c["window"].copy(), c["weights"].copy()
    seen = np.argwhere(w[0, 0] > 0)[:, 0]
    w[1, 0, seen[0]] = -1.0
    win[2, 0, seen[0], 1] = np.nan
    w[3] = 0
    w[3, 0, seen[:2]] = 1
    w[4] = 0
    w[4, 0, seen[:3]] = 1
    win[4, 0, seen[:3]] = win[4, 0, seen[0]]
    w[5, 1, 4] = 0
    win[5, 1, 4] = np.nan
    c.update(window=win, weights=w)
    got, want = _gpu(c), _restate(c)
    assert np.array_equal(got["info"][:, 3], want["info"][:, 3]) and set(np.flatnonzero(want["info"][:, 3])) == set(range(2, 10))
    refused = got["info"][:, 3] != 0
    assert np.array_equal(got["info"][refused], np.tile(np.float32([0, 0, -1, sc.REFUSED]), (8, 1)))
    assert np.array_equal(got["xf"][refused], np.tile(np.eye(4, dtype=np.float32), (8, 1, 1)))
    assert np.array_equal(_bits(got["ja"]), _bits(want["ja"]))
    clean = win.copy()
    clean[5, 1, 4] = 0.0
    again = _gpu(dict(c, window=clean))
    assert all(np.array_equal(_bits(got[f]), _bits(again[f])) for f in got)


# ----------------------------------------------------------------------------- 4. the selection, exactly
def test_select_pose_has_the_restatements_bits():
    rng = np.random.default_rng(3)
    n, k = 7, 4
    ja = rng.normal(size=(n * k, 22)).astype(np.float32)
    xf = rng.normal(size=(n * k, 4, 4)).astype(np.float32)
    xf[:, 3] = [0, 0, 0, 1]
    info = np.abs(rng.normal(size=(n * k, 4))).astype(np.float32)
    info[:, 3] = rng.choice([1, 2, 4, 5], n * k)
    info[4:8, 3] = 4                                       # all refused
    info[8:12, 0], info[8:12, 3] = 1.5, 1                  # a four-way tie
    info[12, 0], info[13, 0], info[12:16, 3] = np.nan, 2.0, 2
    info[17, 0], info[16:20, 3] = info[16, 0], 1           # a tie of the first two, unless a later one is lower
    want = sc.select_pose(ja, xf, info, k)
    assert want[3][1] == -1 and want[3][2] == 0 and want[3][3] != 0
    got = _native.select_pose(_t(ja), _t(xf), _t(info), k)
    torch.cuda.synchronize()
    for g, w_ in zip(got[:3], want[:3]):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w_))
    assert got[3].dtype == torch.int32 and np.array_equal(got[3].cpu().numpy(), want[3])
    one = _native.select_pose(_t(ja[:k]), _t(xf[:k]), _t(info[:k]), k)
    assert np.array_equal(_bits(one[0].cpu().numpy()), _bits(want[0][:1])) and int(one[3][0]) == int(want[3][0])


# ----------------------------------------------------------------------------- 5. deferred checks, graph replay
def test_chain_replays_from_a_graph_and_the_index_check_is_deferred():
    """With an engine in deferred-check mode the three launches synchronise nothing: captured in a graph and replayed they give the
    bits of the eager run, and a cam_rows entry out of range raises from poll_status, not from the call."""
    c = _case("ragged_v3")
    blob, win, rows, table = _blob(c["hm"]), _t(c["window"], torch.float64), _t(c["cam_rows"], torch.int32), _t(c["table"], torch.float64)
    w, mirror, bank, seeds = _t(c["weights"]), _t(c["mirror"], torch.int64), _t(c["bank"]), _t(c["seeds"], torch.float64)
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            def chain(r):
                return pipeline.fit_keypoints_in_views_cold(blob, win, table, r, bank, seeds, w, mirror, engine=eng)

            eager = chain(rows)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                replayed = chain(rows)
            graph.replay()
            torch.cuda.synchronize()
            eng.poll_status()
            bad = rows.clone()
            bad[2, 0] = table.shape[0]
            _native.start_pose_views(blob, win, bad, table, bank, seeds, w, None, mirror, engine=eng)      # no error here ...
            torch.cuda.synchronize()
            with pytest.raises(IndexError):
                eng.poll_status()                     # ... but here
    finally:
        eng.close()
    for e, r in zip(eager, replayed):
        assert torch.equal(e.view(torch.int32), r.view(torch.int32))
    assert bool((eager[3] >= 0).all()) and bool((eager[2][:, 2] >= 1).all())
    with pytest.raises(IndexError):
        _native.start_pose_views(blob, win, bad, table, bank, seeds, w, None, mirror)                       # synchronous without an engine


# ----------------------------------------------------------------------------- 6. the full chain on the 74 hands
@pytest.mark.parametrize("views", ["two", "one"])
def test_full_chain_finds_the_golden_hands(views):
    """test_start_host's yardstick with the kernel's starts and the real ut_fit_pose_views (64 iterations) and ut_select_pose, through
    hand.fit_landmarks_views_cold: exact windows - 74 of 74 within sc.BASIN_MM in two views, at least 72 with the best view alone;
    1 px noise - the selected rms within 1.05 x the float64 label-started fit's + 0.01 px on at least 72."""
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    counts = []
    for noise in (0, 1.0):
        c = sc.golden_case(views, noise)
        ja, xf, info, index = hand.fit_landmarks_views_cold(model, torch.from_numpy(c["window"]).to(DEV), torch.from_numpy(c["cam_rows"]).to(DEV),
                                                            torch.from_numpy(c["table"]), torch.from_numpy(c["weights"]).to(DEV),
                                                            torch.from_numpy(c["mirror"]).to(DEV), max_iters=64)
        res = dict(ja=ja.cpu().numpy(), xf=xf.cpu().numpy(), info=info.cpu().numpy())
        assert ja.shape == (74, 22) and index.dtype == torch.int32 and bool((index >= 0).all())
        counts.append(int((sc.landmark_error(c, res) <= sc.BASIN_MM).sum()) if not noise else int(sc.rms_criterion(c, res).sum()))
    print(f"{views} views: {counts[0]} / 74 within {sc.BASIN_MM} mm on exact windows, {counts[1]} / 74 by the rms criterion at 1 px noise")
    assert counts[0] == 74 if views == "two" else counts[0] >= 72
    assert counts[1] >= 72


# ----------------------------------------------------------------------------- 7. the tracker's calls
def test_tracker_finds_and_follows_a_hand_without_a_start():
    """Hand 1 of frames 200..203 (smooth_cases.recording: two views, 0.5 px): hand_pose_from_window_keypoints_cold finds frame 0 from
    its detections alone, and track_hand_poses_in_views without an init takes the cold result at frame 0 and follows with warm fits;
    every pose within sc.BASIN_MM of its label, every chosen rms within the rule of the cold one."""
    import fit_cases as fc
    import smooth_cases as sm
    from absolutetrack_amd import tracker
    seq = sm.recording(200, 203, 1, 2, 0.5)
    c = seq["views_case"]
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    n_cam = lab["cameras"].shape[0]
    cams = [[pipeline.cameras_for_frame(lab, 200 + t)[int(r) % n_cam] for r in c["cam_rows"][t]] for t in range(4)]
    truth = fc.forward(c["hm"], seq["truth_ja"].astype(np.float64)[:, :20], fc.effective_wrist(seq["truth_xf"].astype(np.float64), c["mirror"], 1.0, np.float64))

    def error(poses):
        res = dict(ja=np.stack([p.joint_angles for p in poses]), xf=np.stack([p.wrist_xform for p in poses]))
        return np.linalg.norm(vc.landmarks(dict(c, mirror=c["mirror"][:len(poses)]), res) - truth[:len(poses)], axis=-1).max(1)

    pose, info, index = tracker.hand_pose_from_window_keypoints_cold(model, cams[0], c["window"][0], 1, c["weights"][0])
    assert 0 <= index < 4 and info.shape == (4,) and pose.hand_confidence == 1.0 and error([pose])[0] <= sc.BASIN_MM
    poses, infos, recovered = tracker.track_hand_poses_in_views(model, cams, c["window"], 1, weights=c["weights"])
    err = error(poses)
    print(f"tracked without a start: worst landmark {err.round(2).tolist()} mm, rms {infos[:, 0].round(3).tolist()} px, recovered {recovered.tolist()}")
    assert recovered.tolist() == [True, False, False, False] and np.all(err <= sc.BASIN_MM)
    assert np.array_equal(infos[0], info) and np.array_equal(poses[0].joint_angles, pose.joint_angles)
    again = tracker.track_hand_poses_in_views(model, cams, c["window"], 1, init=poses[0], weights=c["weights"])
    assert not again[2].any() and np.all(error(again[0]) <= sc.BASIN_MM)
