"""GPU tests of the sequences tracked in one launch (csrc/track_views.hip through ut_track_pose_views, hand.track_landmarks_views,
pipeline.track_keypoints_in_views and the two tracker functions that go through it).

The yardstick is the per-frame chain of the EXISTING entries: _native.fit_pose_views_robust launched frame by frame over the
sequences in lockstep, every launch read back and include/umetrack_hip_track.h's rule applied on the host (`_chain`).  The new
entry is defined as that chain, so every comparison is bit equality of joint_angles, wrist_xf, info and chosen - no tolerance.  The
cold results both sides read come from the existing cold chain (hand._cold_chain), once per case.  tests/test_track_host.py checks
that on every case here the float64 warm / cold rms ratios stay clear of the threshold."""
import functools

import numpy as np
import pytest
import torch

import start_cases as sc
import step_cases as st
import track_cases as tk
from absolutetrack_amd import _native, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7.0


def _t(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _device(k):
    """A case's arrays on the device: dict(blob, win, rows, table, w, mirror, limits, init)."""
    c = k["c"]
    return dict(blob=_t(_native.hand_model_blob(*(c["hm"][f] for f in st.FIELDS))).reshape(-1, 321), win=_t(c["window"], torch.float64),
                rows=_t(c["cam_rows"], torch.int32), table=_t(c["table"], torch.float64), w=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64),
                limits=_t(c["limits"]), init=None if k["init"] is None else (_t(k["init"][0]), _t(k["init"][1])))


def _cold(k, d):
    """The existing cold chain on every row of the case: (ja [n,22], xf [n,4,4], info [n,4], index i32 [n])."""
    return hand._cold_chain(d["blob"], (d["win"], d["rows"], d["table"]), d["w"], d["limits"], d["mirror"], _t(sc.bank()), _t(sc.seeds(), torch.float64),
                            sc.ITERS, 32, k["loss"], k["loss_scale"], k["c"]["t_scale"])


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(case, its device arrays, the cold chain's results or None), once per case.  Leave them unchanged."""
    k = tk.case(name)
    d = _device(k)
    return k, d, _cold(k, d) if k["cold"] else None


def _lengths(k):
    return [k["n_frames"]] * k["n_seq"] if k["lengths"] is None else [int(l) for l in k["lengths"]]


def _chain(k, d, cold, recover_ratio=tk.RECOVER_RATIO, recover_floor=tk.RECOVER_FLOOR_PX):
    """The parent's code: one _native.fit_pose_views_robust launch per frame over the sequences that have a start, read back, the rule
    on the host in Python floats.  dict(ja [n,22], xf [n,4,4], info [n,4], chosen i32 [n]) on the device; rows at or past a length
    keep FILL in ja / xf, 0 in info, -1 in chosen."""
    s_n, t_n = k["n_seq"], k["n_frames"]
    n = s_n * t_n
    lengths = _lengths(k)
    ja, xf = torch.full((n, 22), FILL, device=DEV), torch.full((n, 4, 4), FILL, device=DEV)
    info, chosen = torch.zeros(n, 4, device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV)
    have = [d["init"] is not None] * s_n
    prev_ja, prev_xf = torch.zeros(s_n, 22, device=DEV), torch.zeros(s_n, 4, 4, device=DEV)
    if d["init"] is not None:
        prev_ja.copy_(d["init"][0])
        prev_xf.copy_(d["init"][1])
    cold_info, cold_index = (None, None) if cold is None else (cold[2].cpu(), cold[3].cpu())
    for t in range(t_n):
        live = [s for s in range(s_n) if t < lengths[s]]
        warm, fresh = [s for s in live if have[s]], [s for s in live if not have[s]]
        if warm:
            sel, rows = torch.tensor(warm, device=DEV), torch.tensor([s * t_n + t for s in warm], device=DEV)
            fit = _native.fit_pose_views_robust(d["blob"], d["win"][rows], d["rows"][rows], d["table"], prev_ja[sel], prev_xf[sel], d["w"][rows],
                                                d["limits"], d["mirror"][rows], k["c"]["t_scale"], 32, k["loss"], k["loss_scale"])
            warm_info = fit[2].cpu()
            for j, s in enumerate(warm):
                i = s * t_n + t
                take = False
                if cold is not None:
                    lost = bool(int(warm_info[j, 3]) & _native.UT_FIT_REFUSED) or float(warm_info[j, 0]) > recover_ratio * float(cold_info[i, 0]) + recover_floor
                    take = lost and int(cold_index[i]) >= 0
                if take:
                    ja[i], xf[i], info[i], chosen[i] = cold[0][i], cold[1][i], cold[2][i], tk.COLD
                else:
                    ja[i], xf[i], info[i], chosen[i] = fit[0][j], fit[1][j], fit[2][j], tk.WARM
                prev_ja[s], prev_xf[s] = ja[i], xf[i]
        for s in fresh:
            i = s * t_n + t
            ja[i], xf[i], info[i] = cold[0][i], cold[1][i], cold[2][i]
            have[s] = int(cold_index[i]) >= 0
            chosen[i] = tk.COLD if have[s] else tk.NONE
            prev_ja[s], prev_xf[s] = ja[i], xf[i]
    return dict(ja=ja, xf=xf, info=info, chosen=chosen)


def _track(k, d, cold, rows=None, engine=None, info_fill=None):
    """The entry on a case, into buffers filled with FILL: dict(ja [n,22], xf [n,4,4] - row 3 from the buffer, FILL with xf_stride 12 -,
    info, chosen).  record > 0: both outputs inside [n + 1, record] pose records, whose other floats must stay FILL."""
    n = k["n_seq"] * k["n_frames"]
    stride = k["xf_stride"]
    kw = {}
    if k["record"]:
        rec = torch.full((n + 1, k["record"]), FILL, device=DEV)
        out = (rec[:, :22], rec[:, 22:38])
        kw.update(ja_stride=k["record"], xf_stride=k["record"])
    else:
        out = (torch.full((n + 1, 22), FILL, device=DEV), torch.full((n + 1, stride), FILL, device=DEV))
        kw.update(xf_stride=stride)
    if info_fill is not None:
        kw.update(info=torch.full((n, 4), info_fill, device=DEV), chosen=torch.full((n,), int(info_fill), dtype=torch.int32, device=DEV))
    init = d["init"] or (None, None)
    res = _native.track_pose_views(d["blob"], d["win"], d["rows"] if rows is None else rows, d["table"], k["n_frames"], init[0], init[1], cold, d["w"],
                                   d["limits"], d["mirror"], _t(k["lengths"], torch.int32), k["c"]["t_scale"], 32, k["loss"], k["loss_scale"],
                                   tk.RECOVER_RATIO, tk.RECOVER_FLOOR_PX, out=out, engine=engine, **kw)
    torch.cuda.synchronize()
    assert bool((out[0][n] == FILL).all()) and bool((out[1][n] == FILL).all())        # the guard row
    if k["record"]:
        assert bool((rec[:, 38:] == FILL).all())
    xf = torch.full((n, 16), FILL, device=DEV)
    xf[:, :min(stride, 16)] = out[1][:n, :min(stride, 16)]
    return dict(ja=out[0][:n].contiguous(), xf=xf.reshape(n, 4, 4), info=res[2], chosen=res[3])


def _assert_same(k, got, want, what=""):
    """Bit equality on the rows inside the lengths (the wrist's 12 floats, and row 3 = (0, 0, 0, 1) where the stride has room for it);
    rows at or past a length: pose untouched, info 0, chosen -1."""
    t_n = k["n_frames"]
    live = torch.zeros(k["n_seq"] * t_n, dtype=torch.bool, device=DEV)
    for s, l in enumerate(_lengths(k)):
        live[s * t_n:s * t_n + l] = True
    assert torch.equal(got["chosen"], want["chosen"]), (what, got["chosen"].tolist(), want["chosen"].tolist())
    assert torch.equal(_bits(got["info"]), _bits(want["info"])), what
    assert torch.equal(_bits(got["ja"][live]), _bits(want["ja"][live])), what
    assert torch.equal(_bits(got["xf"][live][:, :3]), _bits(want["xf"][live][:, :3])), what
    if k["xf_stride"] >= 16 or k["record"]:
        assert torch.equal(got["xf"][live][:, 3], torch.tensor([0.0, 0, 0, 1], device=DEV).expand(int(live.sum()), 4)), what
    assert bool((got["ja"][~live] == FILL).all()) and bool((got["xf"][~live] == FILL).all()), what
    assert bool((got["chosen"][~live] == -1).all()) and not bool(got["info"][~live].any()), what


# ----------------------------------------------------------------------------- 1. every case against the per-frame chain
@pytest.mark.parametrize("name", tk.GPU_CASES)
def test_one_launch_has_the_bits_of_the_per_frame_chain(name):
    """Plain sequences (n_seq 1 and 5, n_frames 1, 2, 3 and 12, lengths 12, 7, 3, 1, 0, both hands, a pinhole table, each loss, limits
    given and NULL, t_scale 1000 with xf_stride 12, outputs inside 60-float records), recovery (a wrong init, the documented 64-frame
    loss), starts (no init, cold refused at first, no cold arrays) and a frame with all weights 0."""
    k, d, cold = _prepared(name)
    want = _chain(k, d, cold)
    chosen = want["chosen"].cpu().numpy()
    if name == "wrong_init":
        assert chosen[0] == tk.COLD                                                    # the chain itself recovers at frame 0
    elif name == "loss64":
        recovered = chosen == tk.COLD
        print(f"loss64: the per-frame chain recovers at frames {np.flatnonzero(recovered).tolist()}")
        assert recovered.any()
    elif name == "no_init":
        assert chosen.reshape(2, 4)[:, 0].tolist() == [tk.COLD, tk.COLD] and np.all(chosen.reshape(2, 4)[:, 1:] == tk.WARM)
    elif name == "cold_refused_first":
        assert chosen.tolist() == [tk.NONE, tk.NONE, tk.COLD, tk.WARM]
    elif name == "no_cold":
        assert cold is None and set(chosen.tolist()) == {tk.WARM, -1}
    elif name == "blank_dark_first":
        assert chosen.tolist() == [tk.NONE, tk.NONE, tk.COLD, tk.WARM, tk.WARM, tk.WARM]
    elif name == "blank_frame":
        assert chosen.tolist() == [tk.WARM] * 6 and int(want["info"][3, 3]) & _native.UT_FIT_REFUSED and int(want["info"][4, 3]) & _native.UT_FIT_CONVERGED
        assert torch.equal(want["ja"][3], want["ja"][2]) and torch.equal(want["xf"][3], want["xf"][2])      # the start is carried
    elif name == "five":
        assert set(d["mirror"].tolist()) == {0, 1} and (chosen == -1).sum() == 60 - 23
    got = _track(k, d, cold)
    _assert_same(k, got, want, name)


# ----------------------------------------------------------------------------- 2. a sequence alone, in a batch, padded, in more frames
def test_a_sequence_has_its_bits_alone_in_a_batch_and_in_longer_rows():
    """Sequence 1 of `five` (hand 0, 7 frames): the bits it has in the batch of 5 are those it has alone with NaN behind its length, and
    alone in rows of 16 frames instead of 12."""
    k, d, cold = _prepared("five")
    whole = _track(k, d, cold)
    for t_n in (12, 16):
        c, init, lengths = tk.sequences((tk.FIVE[1],), t_n)
        c["limits"] = k["c"]["limits"]
        one = dict(k, c=c, n_seq=1, n_frames=t_n, lengths=lengths, init=init)
        assert np.isnan(c["window"][7:]).all() and np.isnan(c["weights"][7:]).all()
        d1 = _device(one)
        alone = _track(one, d1, _cold(one, d1))
        assert alone["chosen"].tolist() == [tk.WARM] * 7 + [-1] * (t_n - 7)
        for f in ("ja", "xf", "info", "chosen"):
            assert torch.equal(_bits(alone[f][:7]), _bits(whole[f][12:19])), (t_n, f)


# ----------------------------------------------------------------------------- 3. a bad cam_rows entry in a middle frame
def test_a_bad_camera_row_refuses_its_sequence_alone():
    """cam_rows of frame 3 of sequence 1 points behind the table: synchronous checks raise from the call, deferred ones from
    poll_status; either way sequence 1 writes nothing at all - neither poses nor info nor chosen - and its neighbours are intact."""
    k, d, cold = _prepared("five")
    good = _track(k, d, cold, info_fill=FILL)
    bad = d["rows"].clone()
    bad[12 + 3, 1] = d["table"].shape[0]
    n = 60
    buf = dict(ja=torch.full((n + 1, 22), FILL, device=DEV), xf=torch.full((n + 1, 16), FILL, device=DEV), info=torch.full((n, 4), FILL, device=DEV),
               chosen=torch.full((n,), 7, dtype=torch.int32, device=DEV))
    args = (d["blob"], d["win"], bad, d["table"], 12, d["init"][0], d["init"][1], cold, d["w"], d["limits"], d["mirror"], _t(k["lengths"], torch.int32), 1.0,
            32, k["loss"], k["loss_scale"])

    def check():
        torch.cuda.synchronize()
        mine = slice(12, 24)
        assert all(bool((buf[f][mine] == 7).all()) for f in buf)
        got = dict(ja=buf["ja"][:n], xf=buf["xf"][:n].reshape(n, 4, 4), info=buf["info"], chosen=buf["chosen"])
        for f in got:
            assert torch.equal(_bits(got[f][:12]), _bits(good[f][:12])) and torch.equal(_bits(got[f][24:]), _bits(good[f][24:])), f
        for t in buf.values():
            t.fill_(7)

    with pytest.raises(IndexError):
        _native.track_pose_views(*args, out=(buf["ja"], buf["xf"]), info=buf["info"], chosen=buf["chosen"])
    check()
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            _native.track_pose_views(*args, out=(buf["ja"], buf["xf"]), info=buf["info"], chosen=buf["chosen"], engine=eng)      # no error here ...
            torch.cuda.synchronize()
            with pytest.raises(IndexError):
                eng.poll_status()                         # ... but here
            check()
    finally:
        eng.close()


# ----------------------------------------------------------------------------- 4. graph replay of the whole chain
def test_detections_to_smoothed_poses_replay_from_a_graph():
    """pipeline.track_keypoints_in_views(smooth=True) on 2 x 12 frames - cold chain, track, information, smoother: six launches on one
    stream - with deferred checks: captured and replayed it gives the bits of the eager run, and its track step is the entry's."""
    k, d, cold = _prepared("records")
    bank, seeds = _t(sc.bank()), _t(sc.seeds(), torch.float64)
    step_var = _t(np.tile(np.float32([0.02] * 20 + [0.01] * 3 + [1.0] * 3) ** 2, (1, 1)))
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            def chain():
                r = pipeline.track_keypoints_in_views(d["blob"], d["win"], d["table"], d["rows"], 2, bank, seeds, d["init"][0], d["init"][1], d["w"],
                                                      d["mirror"], loss=k["loss"], loss_scale=k["loss_scale"], smooth=True, step_var=step_var,
                                                      with_sigma=True, engine=eng)
                return r[:4] + r[4] + r[5]

            eager = chain()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                replayed = chain()
            graph.replay()
            torch.cuda.synchronize()
            eng.poll_status()
    finally:
        eng.close()
    assert len(eager) == 12
    for e, r in zip(eager, replayed):
        assert torch.equal(_bits(e), _bits(r))
    want = _track(dict(k, record=0), d, cold)
    for f, e in zip(("ja", "xf", "info", "chosen"), eager):
        assert torch.equal(_bits(e), _bits(want[f])), f
    assert bool((eager[10][..., 3].to(torch.int64) & _native.UT_SMOOTH_OK).bool().all())


# ----------------------------------------------------------------------------- 5. the tracker's functions
def _same_poses(a, b):
    return len(a) == len(b) and all(np.array_equal(p.joint_angles.view(np.uint32), q.joint_angles.view(np.uint32)) and
                                    np.array_equal(p.wrist_xform.view(np.uint32), q.wrist_xform.view(np.uint32)) and
                                    p.hand_confidence == q.hand_confidence for p, q in zip(a, b))


def test_rerouted_tracker_functions_return_what_their_loops_returned():
    """tracker.track_hand_poses_in_views (no init; a wrong init, recovered from at frame 0; no cold result for the first two frames)
    and tracker.smooth_hand_poses_in_views on hand 1 of frames 200..205 against in-test copies of their per-frame loops: the cases
    blank_no_init, blank_wrong_init, blank_dark_first and blank_frame of track_cases."""
    k = tk.case("blank_frame")
    c = k["c"]
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    n_cam = lab["cameras"].shape[0]
    cams = [[pipeline.cameras_for_frame(lab, 200 + t)[int(r) % n_cam] for r in c["cam_rows"][t]] for t in range(6)]
    label = tracker.SingleHandPose(k["init"][0][0], k["init"][1][0])
    far = tk.turned(k["init"])
    dark = c["weights"].copy()
    dark[:2] = 0
    for init, weights, first in ((None, c["weights"], True), (tracker.SingleHandPose(far[0][0], far[1][0]), c["weights"], True), (None, dark, False)):
        new = tracker.track_hand_poses_in_views(model, cams, c["window"], 1, init=init, weights=weights)
        old = tk.former_track_loop(model, cams, c["window"], 1, init, tracker.RECOVER_RATIO, weights)
        assert _same_poses(new[0], old[0]) and np.array_equal(new[1].view(np.uint32), old[1].view(np.uint32)) and np.array_equal(new[2], old[2])
        assert new[2].dtype == np.bool_ and new[1].dtype == np.float32 and bool(new[2][0]) == first and int(new[1][3, 3]) & _native.UT_FIT_REFUSED
    assert new[2].tolist() == [False, False, True, False, False, False]
    # the smoother's fits: the warm chain without cold results
    step = hand.step_sigma_from_rates(2.0, 1.0, 100.0, 30.0)
    new = tracker.smooth_hand_poses_in_views(model, cams, c["window"], 1, label, step, weights=c["weights"])
    pose, fits = label, []
    for t in range(6):
        pose = tracker.refine_hand_pose_in_views(model, cams[t], c["window"][t], 1, pose, c["weights"][t])[0]
        fits.append(pose)
    tables = [tracker._window_inputs("old", cams[t], c["window"][t], c["weights"][t], (2, 21, 2))[0] for t in range(6)]
    ja = torch.from_numpy(np.stack([np.asarray(p.joint_angles, np.float32) for p in fits]))
    xf = torch.from_numpy(np.stack([np.asarray(p.wrist_xform, np.float32) for p in fits]))
    rows = torch.arange(12, dtype=torch.int32).reshape(6, 2)
    mirror = tracker._mirror_flag(1)
    unc = hand.pose_uncertainty_views(model, ja, xf, torch.from_numpy(c["window"]), rows, torch.from_numpy(np.concatenate(tables)),
                                      weights=torch.from_numpy(c["weights"]), mirror=mirror.expand(6))
    sja, sxf, info, sigma = hand.smooth_poses(model, ja, xf, unc, step, mirror=mirror, return_sigma=True)
    old = [tracker.SingleHandPose(sja[t].numpy(), sxf[t].numpy(), fits[t].hand_confidence) for t in range(6)]
    assert _same_poses(new[0], old) and np.array_equal(new[1].view(np.uint32), info.numpy().view(np.uint32))
    assert np.array_equal(new[2].view(np.uint32), sigma.numpy().view(np.uint32))
