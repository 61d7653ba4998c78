"""GPU tests of the poses smoothed over a sequence (csrc/smooth.hip through ut_smooth_pose_sequence and hand.smooth_poses) against
the float64 dense solve and the float32 recursions of tests/smooth_cases.py, which tests/test_smooth_host.py checks.  The shapes
are n_seq 1 and 5 and T 1, 2, 3 and 12: sub-sequences of frames 200..211 of recording_00, hand 0, fitted in two views.

Bounds by smooth_cases.bounds_from - DESIGN's rule: the project's bounds, or step_cases.FLOAT32_FACTOR x the worst distance of the
two float32 restatements from float64 on the sequence, computed here from the restatements, never from the kernel's output, and
printed next to the kernel's distance.  Measured figures: DESIGN.md, "Poses smoothed over a sequence"."""
import ctypes

import numpy as np
import pytest
import torch

import smooth_cases as sm
import step_cases as st
from absolutetrack_amd import _native, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("ja", "xf", "sigma", "info")
LENGTHS = (12, 7, 3, 1, 0)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pad(a, frames, fill):
    a = np.asarray(a, np.float32)
    out = np.full((frames,) + a.shape[1:], fill, np.float32)
    out[:len(a)] = a
    return out


def _batch(seqs, frames, fill=np.nan, n_var=None, centre=True, weight=True):
    """Sequences (each at most `frames` long) as one batch: the tensors of _native.smooth_pose_sequence and its keywords.  The
    padding behind a sequence's length is `fill` everywhere but in the poses, which are finite (copied through)."""
    ja = np.stack([_pad(s["ja"], frames, 0.25) for s in seqs])
    xf = np.stack([_pad(s["xf"], frames, 0.5) for s in seqs])
    info = np.stack([_pad(s["pose_info"], frames, fill) for s in seqs])
    piv = np.stack([_pad(s["pivot"], frames, fill) for s in seqs])
    kw = dict(lengths=_t(np.array([len(s["ja"]) for s in seqs]), torch.int32), t_scale=seqs[0]["t_scale"])
    if weight:
        kw["frame_weight"] = _t(np.stack([_pad(np.ones(len(s["ja"])) if s.get("weight") is None else s["weight"], frames, fill) for s in seqs]))
    if centre:
        kw["centre"] = _t(np.stack([np.zeros(3, np.float32) if s.get("centre") is None else s["centre"] for s in seqs]))
    q = np.stack([s["step_var"] for s in seqs])[:n_var]          # n_var 1: one row for every sequence
    return (_t(ja), _t(xf), _t(info), _t(piv), _t(q)), kw


def _run(seqs, frames, **how):
    """The batch on the GPU: per sequence the dict smooth_cases.smooth returns, cut to the sequence's length, and the raw arrays."""
    more = {k: how.pop(k) for k in ("param_sigma", "info", "out", "workspace") if k in how}
    args, kw = _batch(seqs, frames, **how)
    out = _native.smooth_pose_sequence(*args, **kw, **dict(dict(param_sigma=True, info=True), **more))
    torch.cuda.synchronize()
    raw = dict(zip(OUT, (None if o is None else o.cpu().numpy() for o in out)))
    return [{k: raw[k][i, :len(s["ja"])] for k in OUT if raw[k] is not None} for i, s in enumerate(seqs)], raw


def _show(what, d, d32, tol):
    print(f"{what}: " + ", ".join(f"{k} GPU {d[k]:.2e} float32 {d32[k]:.2e} bound {tol[k]:.2e}" for k in d))


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("scale", sm.Q_SCALES)
def test_sequences_match_float64_across_the_step_variances(scale):
    """The five named sequences of 12 frames (gaps at the first, a middle and the last frame; a rank-1 H; centre NULL; metres) with
    the step variances x scale, each alone (n_seq 1, n_var 1): poses, param_sigma and info within the bounds."""
    for name in sm.CASES:
        seq = sm.scaled(sm.case(name), scale)
        want = sm.smooth(seq)
        d32 = sm.float32_distance(seq, want)
        got = _run([seq], 12, centre=seq.get("centre") is not None, weight=seq.get("weight") is not None)[0][0]
        d, tol = sm.distance(seq, got, want), sm.bounds_from(d32)
        _show(f"{name} q x {scale:g}", d, d32, tol)
        assert sm.within(d, tol), (name, scale, d, tol)


@pytest.mark.parametrize("frames", [1, 2, 3])
def test_short_sequences_match_float64(frames):
    """T = 1, 2, 3 in a batch of 5 with the ragged lengths of LENGTHS capped at T; T = 1 moves nothing and its sigma is
    sqrt(diag H'^-1)."""
    b = sm.case("gaps")
    seqs = [sm.cut(b, slice(o, o + min(n, frames))) for o, n in zip((1, 2, 3, 4, 6), LENGTHS)]
    got = _run(seqs, frames)[0]
    for s, g in zip(seqs, got):
        if len(s["ja"]) == 0:
            continue
        want = sm.smooth(s)
        d, d32 = sm.distance(s, g, want), sm.float32_distance(s, want)
        tol = sm.bounds_from(d32)
        _show(f"T {frames} length {len(s['ja'])}", d, d32, tol)
        assert sm.within(d, tol), (frames, d, tol)
        if len(s["ja"]) == 1:
            assert np.array_equal(_bits(g["ja"]), _bits(s["ja"])) and np.array_equal(_bits(g["info"][:, :2]), _bits(np.zeros((1, 2))))


# ----------------------------------------------------------------------------- 2. batches, padding, in place
def _ragged():
    b = sm.case("gaps")
    return [sm.cut(b, slice(0, n), step_var=(b["step_var"] * (1 + i)).astype(np.float32)) for i, n in enumerate(LENGTHS)]


def test_a_sequence_does_not_depend_on_its_batch_nor_on_its_padding():
    """Five sequences of lengths 12, 7, 3, 1, 0 (n_var = n_seq, centre given, weights given): each has the bits it has alone, with
    NaN and with finite padding behind its length, and in 16 frames instead of 12; frames at or past the length are copied through
    with status 0, sigma 0 and info 0."""
    seqs = _ragged()
    got, raw = _run(seqs, 12)
    for frames, fill in ((12, 7.0), (16, np.nan)):
        again = _run(seqs, frames, fill=fill)[0]
        for a, b in zip(got, again):
            assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in OUT)
    for i, s in enumerate(seqs):
        n = len(s["ja"])
        if n:
            alone = _run([s], n)[0][0]
            assert all(np.array_equal(_bits(alone[k]), _bits(got[i][k])) for k in OUT), i
            want = sm.smooth(s)
            assert np.array_equal(got[i]["info"][:, 3], want["info"][:, 3])
        assert np.array_equal(raw["ja"][i, n:], np.full((12 - n, 22), 0.25, np.float32))
        assert np.array_equal(raw["xf"][i, n:, :3], np.full((12 - n, 3, 4), 0.5, np.float32)) and np.all(raw["xf"][i, n:, 3] == (0, 0, 0, 1))
        assert not raw["sigma"][i, n:].any() and not raw["info"][i, n:].any()
    assert (got[0]["info"][:, 3] == np.where(np.isin(np.arange(12), (0, 5, 11)), sm.OK | sm.GAP, sm.OK)).all()
    shared = [dict(s, step_var=seqs[0]["step_var"]) for s in seqs]                         # n_var 1 against n_var = n_seq
    one, each = _run(shared, 12, n_var=1)[1], _run(shared, 12)[1]
    assert all(np.array_equal(_bits(one[k]), _bits(each[k])) for k in OUT)


def test_in_place_and_strided_outputs_have_the_separate_bits():
    """The outputs in the inputs' own buffers - the angles inside pose records of 60 floats, the wrists as 12 floats at xf_stride 12
    and t_scale 1000 - and without param_sigma: the bits of separate packed outputs, nothing written around them."""
    seqs = [sm.cut(sm.case("metres"), slice(0, n)) for n in LENGTHS]
    got, raw = _run(seqs, 12)
    args, kw = _batch(seqs, 12)
    rec = torch.full((5 * 12, 60), -3.0, device=DEV)
    rec[:, 3:25] = args[0].reshape(-1, 22)
    ja, xf = rec[:, 3:25], args[1].reshape(-1, 16)[:, :12].contiguous()
    out = _native.smooth_pose_sequence(ja, xf, *args[2:], **kw, n_seq=5, n_frames=12, ja_stride=60, xf_stride=12, out=(ja, xf),
                                       ja_out_stride=60, xf_out_stride=12, param_sigma=False, info=True)
    torch.cuda.synchronize()
    assert out[2] is None and kw["t_scale"] == 1000.0
    r = rec.cpu().numpy()
    assert np.array_equal(_bits(r[:, 3:25]), _bits(raw["ja"].reshape(-1, 22)))
    assert np.array_equal(_bits(xf.cpu().numpy()), _bits(raw["xf"].reshape(-1, 16)[:, :12]))
    assert np.all(r[:, :3] == -3.0) and np.all(r[:, 25:] == -3.0)
    assert np.array_equal(_bits(out[3].cpu().numpy()), _bits(raw["info"]))


# ----------------------------------------------------------------------------- 3. statuses and arguments
def test_singular_and_refused_write_what_the_header_says():
    """free: no frame observes the index finger - SINGULAR, poses copied through, sigma +inf, info 0 0 pivot status; freed: one
    frame observes it - OK.  Refusals (NaN pose, NaN H at a positive weight, negative weight, zero step variance, a bad length):
    poses copied through, sigma 0, info 0 0 0 REFUSED; a NaN H at weight 0 is not read."""
    free, freed = sm.case("free"), sm.case("freed")
    got = _run([free, freed], 12)[0]
    want = sm.smooth(free)
    assert (got[0]["info"][:, 3] == sm.SINGULAR).all() and np.isinf(got[0]["sigma"]).all() and not got[0]["info"][:, :2].any()
    assert np.array_equal(_bits(got[0]["ja"]), _bits(free["ja"])) and np.array_equal(_bits(got[0]["xf"][:, :3]), _bits(free["xf"][:, :3]))
    assert np.abs(got[0]["info"][:, 2] - want["info"][:, 2]).max() <= sm.bounds_from(sm.float32_distance(freed))["pivot"]
    assert got[0]["info"][11, 2] <= sm.uc.MIN_PIVOT
    assert (got[1]["info"][:, 3] == sm.OK).all() and np.isfinite(got[1]["sigma"]).all()

    b = sm.case("gaps")
    bad = []
    for what in ("pose", "info", "weight", "var", "ok_nan_at_gap"):
        s = sm.cut(b, slice(0, 12))
        if what == "pose":
            s["ja"][4, 7] = np.nan
        elif what == "info":
            s["pose_info"][4, 100] = np.nan
        elif what == "weight":
            s["weight"][2] = -1.0
        elif what == "var":
            s["step_var"] = s["step_var"].copy()
            s["step_var"][25] = 0.0
        else:
            s["pose_info"][5] = np.nan
            s["pivot"][5] = np.nan
        bad.append(s)
    got, raw = _run(bad, 12)
    for s, g in zip(bad[:4], got[:4]):
        assert (g["info"] == np.array([0, 0, 0, sm.REFUSED], np.float32)).all() and not g["sigma"].any()
        assert np.array_equal(_bits(g["ja"]), _bits(s["ja"])) and np.array_equal(_bits(g["xf"][:, :3]), _bits(s["xf"][:, :3]))
    assert all(np.array_equal(_bits(got[4][k]), _bits(_run([b], 12)[0][0][k])) for k in OUT)
    args, kw = _batch([b, b], 12)
    kw["lengths"] = _t(np.array([13, -1]), torch.int32)
    out = _native.smooth_pose_sequence(*args, **kw, param_sigma=True)
    torch.cuda.synchronize()
    assert bool((out[3][..., 3] == sm.REFUSED).all()) and not bool(out[2].any()) and torch.equal(out[0], args[0])


def test_invalid_arguments_launch_nothing_and_name_the_argument():
    lib = _native.load_library()
    args, kw = _batch([sm.case("plain")], 12)
    ws = torch.full((12, sm.WORK), -7.0, device=DEV)
    outs = [torch.full(s, -7.0, device=DEV) for s in ((12, 22), (12, 16), (12, 26), (12, 4))]
    good = dict(ja=args[0].data_ptr(), ja_stride=22, xf=args[1].data_ptr(), xf_stride=16, info=args[2].data_ptr(), piv=args[3].data_ptr(),
                q=args[4].data_ptr(), n_var=1, t_scale=1.0, n_seq=1, n_frames=12, ws=ws.data_ptr(), oja=outs[0].data_ptr(), oja_stride=22,
                oxf=outs[1].data_ptr(), oxf_stride=16)

    def call(**change):
        a = dict(good, **change)
        rc = lib.ut_smooth_pose_sequence(None, a["ja"], a["ja_stride"], a["xf"], a["xf_stride"], a["info"], a["piv"], None, None, None, a["q"],
                                         a["n_var"], ctypes.c_float(a["t_scale"]), a["n_seq"], a["n_frames"], a["ws"], a["oja"], a["oja_stride"],
                                         a["oxf"], a["oxf_stride"], outs[2].data_ptr(), outs[3].data_ptr(), None)
        return rc, lib.ut_last_error(None).decode()

    for change, word in ((dict(ja=None), "joint_angles"), (dict(xf=None), "wrist_xf"), (dict(info=None), "pose_info"), (dict(piv=None), "pivot"),
                         (dict(q=None), "step_var"), (dict(ws=None), "workspace"), (dict(oja=None), "joint_angles_out"),
                         (dict(oxf=None), "wrist_xf_out"), (dict(ja_stride=21), "stride"), (dict(xf_stride=11), "stride"),
                         (dict(oja_stride=21), "stride"), (dict(oxf_stride=11), "stride"), (dict(n_var=2), "n_var"), (dict(n_var=0), "n_var"),
                         (dict(n_frames=0), "n_frames"), (dict(n_seq=-1), "n_seq"), (dict(t_scale=0.0), "t_scale"),
                         (dict(t_scale=float("nan")), "t_scale"), (dict(t_scale=float("inf")), "t_scale"), (dict(n_seq=0, n_frames=0), "n_frames")):
        rc, msg = call(**change)
        assert rc == -1 and msg.startswith("ut_smooth_pose_sequence: ") and word in msg, (change, rc, msg)
    assert call(n_seq=0)[0] == 0
    torch.cuda.synchronize()
    assert bool((ws == -7.0).all()) and all(bool((o == -7.0).all()) for o in outs)          # nothing was launched
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert not bool((outs[3] == -7.0).any())


# ----------------------------------------------------------------------------- 4. the Python layer and graphs
def test_hand_smooth_poses_is_the_native_entry():
    """hand.smooth_poses on CPU tensors with a leading dimension: the native entry's bits with the default centre (the mean of the
    landmarks' rest positions) and step_sigma squared in float32; step_sigma_from_rates divides rates by the frame rate."""
    weight = sm.case("gaps")["weight"]
    sigma = np.sqrt(sm.case("plain")["step_var"]).astype(np.float32)
    seqs = [dict(sm.case(name), weight=weight, step_var=sigma * sigma) for name in ("plain", "rank")]
    want = _run(seqs, 12)[1]
    model = pipeline.hand_model_from_labels(pipeline.load_labels())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rates = hand.step_sigma_from_rates(0.3, 0.2, 150.0, 30.0)
    assert rates.shape == (26,) and torch.allclose(rates, torch.tensor([0.01] * 20 + [0.2 / 30] * 3 + [5.0] * 3))
    stack = lambda k: t(np.stack([s[k] for s in seqs]))
    out = hand.smooth_poses(model, stack("ja"), stack("xf"), (stack("pose_info"), stack("pivot")), t(sigma), frame_weight=t(np.stack([weight] * 2)),
                            mirror=torch.zeros(2, dtype=torch.int64), return_sigma=True)
    assert len(out) == 4 and out[0].shape == (2, 12, 22) and out[1].shape == (2, 12, 4, 4) and out[2].shape == (2, 12, 4) and out[3].shape == (2, 12, 26)
    for got, k in zip(out, ("ja", "xf", "info", "sigma")):
        assert np.array_equal(_bits(got.numpy()), _bits(want[k])), k
    assert len(hand.smooth_poses(model, stack("ja"), stack("xf"), (stack("pose_info"), stack("pivot")), t(sigma))) == 3


def test_replays_from_a_captured_graph():
    """The entry has no status word and allocates nothing: captured under torch.cuda.graph on one batch and replayed on another, it
    leaves the eager bits."""
    first, then = _batch(_ragged(), 12, fill=0.0)[0], _batch([sm.case("plain")] * 5, 12, fill=0.0)[0]
    kw = _batch(_ragged(), 12)[1]
    live = [a.clone() for a in first]
    ws = torch.zeros((60, sm.WORK), device=DEV)

    def buffers():
        return dict(out=(torch.zeros((5, 12, 22), device=DEV), torch.zeros((5, 12, 4, 4), device=DEV)), param_sigma=torch.zeros((5, 12, 26), device=DEV),
                    info=torch.zeros((5, 12, 4), device=DEV))

    eager, replayed = buffers(), buffers()
    _native.smooth_pose_sequence(*live, **kw, **replayed, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.smooth_pose_sequence(*live, **kw, **replayed, workspace=ws)
    for a, b in zip(live, then):
        a.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    _native.smooth_pose_sequence(*live, **kw, **eager, workspace=ws)
    torch.cuda.synchronize()
    for a, b in ((eager["out"][0], replayed["out"][0]), (eager["out"][1], replayed["out"][1]), (eager["param_sigma"], replayed["param_sigma"]),
                 (eager["info"], replayed["info"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool((eager["info"][0, :, 3] >= 1).all())


def _chain_inputs():
    """The detections behind smooth_cases.base() as the tensors of pipeline.smooth_fitted_sequence: 2 sequences of 6 frames, every
    fit started at its label."""
    b = sm.base()
    c = b["views_case"]
    blob = _t(_native.hand_model_blob(*(c["hm"][k] for k in st.FIELDS))).reshape(-1, 321)
    args = (blob, _t(c["window"], torch.float64), _t(c["table"], torch.float64), _t(c["cam_rows"], torch.int32), _t(b["truth_ja"]), _t(b["truth_xf"]),
            _t(b["step_var"]).reshape(1, 26), 2)
    return b, args, dict(weights=_t(c["weights"]), mirror=_t(c["mirror"], torch.int64), with_sigma=True)


def test_the_three_launch_chain_replays_from_a_captured_graph():
    """pipeline.smooth_fitted_sequence - fit, information, smoother on one stream - captured under torch.cuda.graph with deferred
    checks and replayed on other detections: the eager bits.  Its smoothed poses are the native entry's on the chain's own fits, and
    they lie closer to the labels than the fits."""
    b, args, kw = _chain_inputs()
    other = args[1] + 0.25
    win = args[1].clone()
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            run = lambda: pipeline.smooth_fitted_sequence(args[0], win, *args[2:], **kw, engine=eng)
            run()                                         # every lazy initialisation happens before the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                replayed = run()
            win.copy_(other)
            graph.replay()
            torch.cuda.synchronize()
            replayed = [t.clone() for t in replayed[:4]] + [t.clone() for t in replayed[4]]
            eager = run()
            eager = list(eager[:4]) + list(eager[4])
            torch.cuda.synchronize()
            win.copy_(args[1])
            first = run()
            torch.cuda.synchronize()
            eng.poll_status()
    finally:
        eng.close()
    for a, r in zip(eager, replayed):
        assert torch.equal(a.view(torch.int32), r.view(torch.int32))
    ja, xf, info, sigma, fit = first
    assert ja.shape == (2, 6, 22) and xf.shape == (2, 6, 4, 4) and info.shape == (2, 6, 4) and sigma.shape == (2, 6, 26)
    assert bool((info[..., 3] == sm.OK).all()) and bool((fit[2][:, 3] == 1).all())
    seq = sm.cut(b, slice(0, 12), centre=None)
    err = lambda j, x: sm.rms_to_truth(seq, dict(ja=j.reshape(12, 22).cpu().numpy(), xf=x.reshape(12, 4, 4).cpu().numpy()))[0]
    print(f"fits {err(fit[0], fit[1]):.3f} mm -> smoothed {err(ja, xf):.3f} mm")
    assert err(ja, xf) < err(fit[0], fit[1])


def test_tracker_smooths_one_hand_through_a_list_of_frames():
    """tracker.smooth_hand_poses_in_views on the 12 frames behind smooth_cases.base(): per-frame cameras and detections of hand 0,
    fits warm-started frame by frame from the first label, one uncertainty and one smoother launch: 12 poses that lie closer to the
    labels than the frame-by-frame fits, info and sigmas of the smoother."""
    b = sm.base()
    c = b["views_case"]
    lab = pipeline.load_labels()
    model = pipeline.hand_model_from_labels(lab)
    cams = [[pipeline.cameras_for_frame(lab, 200 + t)[int(r) % 4] for r in c["cam_rows"][t]] for t in range(12)]
    init = tracker.SingleHandPose(joint_angles=b["truth_ja"][0], wrist_xform=b["truth_xf"][0], hand_confidence=1.0)
    sigma_step = np.sqrt(b["step_var"])
    poses, info, sigma = tracker.smooth_hand_poses_in_views(model, cams, c["window"], 0, init, sigma_step, weights=c["weights"])
    assert len(poses) == 12 and info.shape == (12, 4) and sigma.shape == (12, 26) and (info[:, 3] == sm.OK).all() and np.isfinite(sigma).all()
    fits, pose = [], init
    for t in range(12):
        pose = tracker.refine_hand_pose_in_views(model, cams[t], c["window"][t], 0, pose, c["weights"][t])[0]
        fits.append(pose)
    seq = sm.cut(b, slice(0, 12))
    err = lambda ps: sm.rms_to_truth(seq, dict(ja=np.stack([p.joint_angles for p in ps]), xf=np.stack([p.wrist_xform for p in ps])))[0]
    print(f"fits {err(fits):.3f} mm -> smoothed {err(poses):.3f} mm")
    assert err(poses) < err(fits)
