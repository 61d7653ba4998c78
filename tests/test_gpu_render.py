"""GPU tests of the rendered hand (csrc/render.hip through ut_project_points / ut_render_mesh).

Projection: against the reference's own numbers (tests/golden/projection_rec00.npz) to 1e-9 px / 1e-9 mm.

Render: against the float64 yardstick of tests/render_cases.py on all label poses of recording_00, the recording's mesh, in
their own crop cameras (crop_plan_on_device), on the fp32 vertices ut_skin_mesh gives.  A pixel is left out only where the
yardstick itself says the answer hangs on less than float32 can hold: its centre within DELTA_PX = 2.2e-5 px of an edge of
a non-skipped triangle, or its two nearest surfaces closer than EPS_MM = 1.4e-2 mm.  Both are 4 x the largest disagreement
of the numpy float32 restatement with float64, measured on the CPU over the same 738 poses / 1476 crops: edge distance
5.28e-6 px, depth 3.44e-3 mm.  The excluded share must stay below 0.5 % of the covered pixels in every crop (measured on the
CPU: at most 0.16 %, mean 0.02 %).  Everywhere else: the same triangle, the same background, depth within EPS_MM, shade
within one grey level."""
import os

import numpy as np
import pytest
import torch

import mesh_cases as mc
import render_cases as rc
from absolutetrack_amd import _native, arch, geometry, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def labels():
    return pipeline.load_labels()


@pytest.fixture(scope="module")
def hm_t(labels):
    v, t, w = mc.load_mesh("rec00")
    return pipeline.hand_model_from_labels(labels)._replace(mesh_vertices=torch.from_numpy(v), mesh_triangles=torch.from_numpy(t),
                                                            dense_bone_weights=torch.from_numpy(w))


@pytest.fixture(scope="module")
def scene(labels, hm_t):
    """All confident label poses, their crop cameras from the device planner, their fp32 vertices and one render of all."""
    n_frames = labels["joint_angles"].shape[0]
    plan = pipeline.crop_plan_on_device(labels, hm_t, range(n_frames), DEV)
    c = pipeline.label_candidates(labels, range(n_frames))
    assert plan["sample_range"].shape[0] == len(c["hand_idx"]) == 738          # every label pose has a view
    mesh = hand.device_mesh(hm_t, torch.device(DEV))
    blob = hand.device_blob(hm_t, torch.device(DEV))
    verts = _native.skin_mesh(mesh, blob, _t(c["joint_angles"]), _t(c["wrist_xf"]), mirror=_t(c["hand_idx"]))
    depth, tri, shade = _native.render_mesh(mesh, verts, plan["crop_params"], plan["sample_range"])
    torch.cuda.synchronize()
    return dict(mesh=mesh, blob=blob, verts=verts, crop_params=plan["crop_params"], sample_range=plan["sample_range"],
                hand=c["hand_idx"], depth=depth, tri=tri, shade=shade, triangles=mc.load_mesh("rec00")[1])


# ----------------------------------------------------------------------------- projection
def test_projection_matches_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "projection_rec00.npz"))
    n_f, n = g["c2w"].shape[0], g["landmarks"].shape[0]
    table = np.stack([geometry.pack_source_camera(g["cams"][ci, 2:4], g["cams"][ci, 4:6], g["cams"][ci, 6:14], g["c2w"][k, ci])
                      for k in range(n_f) for ci in range(4)])
    rows = (g["case_frame"][:, None] * 4 + np.arange(4)[None]).astype(np.int32)
    w, h = int(g["cams"][0, 0]), int(g["cams"][0, 1])
    win, ez, flags = _native.project_points(_t(g["landmarks"]), _t(rows), _t(table), w, h)
    torch.cuda.synchronize()
    win, ez, flags = win.cpu().numpy(), ez.cpu().numpy(), flags.cpu().numpy()
    err, err_z = np.abs(win - g["window"]).max(), np.abs(ez - g["eye_z"]).max()
    print(f"ut_project_points vs the reference, {n} x 4 x 21 points: window {err:.3e} px, z {err_z:.3e} mm")
    assert win.shape == (n, 4, 21, 2) and err <= 1e-9 and err_z <= 1e-9
    want = (g["eye_z"] > 0).astype(np.uint8) | (((g["window"] >= 0).all(-1) & (g["window"][..., 0] < w) & (g["window"][..., 1] < h)).astype(np.uint8) << 1)
    assert np.array_equal(flags, want) and len(np.unique(want)) == 4
    # strided points (records), an unused view, and the tracker's helper
    rec = torch.zeros(n, 123, device=DEV)
    rec[:, 60:] = _t(g["landmarks"]).reshape(n, 63)
    rows2 = rows.copy()
    rows2[::3, 2] = -1
    win2, ez2, fl2 = pipeline.project_keypoints(rec[:, 60:], _t(table), _t(rows2), (w, h), n_points=21, point_stride=123)
    keep = rows2 >= 0
    assert np.array_equal(win2.cpu().numpy()[keep], win[keep]) and np.array_equal(fl2.cpu().numpy()[keep], flags[keep])
    assert (win2.cpu().numpy()[~keep] == 0).all() and (fl2.cpu().numpy()[~keep] == 0).all() and (ez2.cpu().numpy()[~keep] == 0).all()
    cams = []
    for ci in range(4):
        js = dict(zip(pipeline._CAM_FIELDS, g["cams"][ci]))
        js["DistortionModel"] = "FishEye62"
        js["ImageSizeX"], js["ImageSizeY"] = int(js["ImageSizeX"]), int(js["ImageSizeY"])
        cams.append(geometry.read_camera_from_json(js).copy(camera_to_world_xf=g["c2w"][int(g["case_frame"][5]), ci]))
    assert np.array_equal(tracker.project_landmarks(cams, g["landmarks"][5]), win[5])
    from lib.tracker.perspective_crop import project_landmarks as dropin
    assert dropin is tracker.project_landmarks
    # a row outside the table: IndexError, and the device stays usable
    rows2[0, 0] = table.shape[0]
    with pytest.raises(IndexError, match="ut_project_points"):
        _native.project_points(_t(g["landmarks"]), _t(rows2), _t(table), w, h)
    again, _, _ = _native.project_points(_t(g["landmarks"]), _t(rows), _t(table), w, h)
    assert np.array_equal(again.cpu().numpy(), win)


def test_projection_into_crop_cameras(scene):
    crop = scene["crop_params"].cpu().numpy()
    sr = scene["sample_range"].cpu().numpy()
    rows = pipeline.view_rows(torch.arange(crop.shape[0], device=DEV), scene["sample_range"])
    assert rows.shape == (738, 2) and int((rows >= 0).sum()) == crop.shape[0]
    win, ez, flags = _native.project_points(scene["verts"], rows, scene["crop_params"], 96, 96)
    win, ez, rows = win.cpu().numpy(), ez.cpu().numpy(), rows.cpu().numpy()
    verts = scene["verts"].cpu().numpy().astype(np.float64)
    worst = worst_z = 0.0
    for i in range(0, 738, 5):
        for v in range(sr[i, 1] - sr[i, 0]):
            cam = tracker._crop_camera_from_row(crop[sr[i, 0] + v], None, None, 96)
            eye = cam.world_to_eye(verts[i])
            worst = max(worst, float(np.abs(cam.eye_to_window(eye) - win[i, v]).max()))
            worst_z = max(worst_z, float(np.abs(eye[:, 2] - ez[i, v]).max()))
    print(f"crop cameras vs geometry.PinholePlaneCameraModel: window {worst:.3e} px, z {worst_z:.3e} mm")
    assert worst <= 1e-9 and worst_z <= 1e-9


# ----------------------------------------------------------------------------- render against float64
def test_render_matches_float64_yardstick(scene):
    """See the module docstring for DELTA_PX, EPS_MM and the 0.5 % cap."""
    crop = scene["crop_params"].cpu().numpy()
    sr = scene["sample_range"].cpu().numpy()
    verts = scene["verts"].cpu().numpy()
    depth, tri, shade = scene["depth"].cpu().numpy(), scene["tri"].cpu().numpy(), scene["shade"].cpu().numpy()
    worst = dict(share=0.0, depth=0.0, shade=0, tri=0, bg=0)
    compared = covered = 0
    mirror_checked = 0
    for i in range(sr.shape[0]):
        for c in range(sr[i, 0], sr[i, 1]):
            y = rc.rasterise(verts[i], scene["triangles"], crop[c], delta=rc.DELTA_PX, eps=rc.EPS_MM)
            ok = ~y["excluded"]
            share = float((y["excluded"] & (y["tri"] >= 0)).sum()) / y["covered"]
            worst["share"] = max(worst["share"], share)
            hit = ok & (y["tri"] >= 0)
            worst["tri"] += int((tri[c][ok] != y["tri"][ok]).sum())
            worst["bg"] += int(((tri[c] < 0) != (y["tri"] < 0))[ok].sum())
            same = hit & (tri[c] == y["tri"])
            if same.any():
                worst["depth"] = max(worst["depth"], float(np.abs(depth[c][same].astype(np.float64) - y["depth"][same]).max()))
                worst["shade"] = max(worst["shade"], int(np.abs(shade[c][same].astype(int) - y["shade"][same].astype(int)).max()))
            assert np.isinf(depth[c][tri[c] < 0]).all() and (shade[c][tri[c] < 0] == 0).all()
            compared += int(ok.sum())
            covered += y["covered"]
            if scene["hand"][i] == 1 and mirror_checked < 40 and not y["excluded"].any():
                assert int((tri[c] >= 0).sum()) == y["covered"]         # a right hand in its x-mirrored camera: same coverage
                lit = tri[c] >= 0
                assert abs(float(shade[c][lit].mean()) - float(y["shade"][lit].mean())) < 0.5      # and not inverted shading
                mirror_checked += 1
    print(f"{crop.shape[0]} crops, {covered} covered pixels, {compared} compared: wrong triangle {worst['tri']}, wrong background "
          f"{worst['bg']}, depth {worst['depth']:.3e} mm (bound {rc.EPS_MM:.1e}), shade {worst['shade']} levels, largest excluded share "
          f"{worst['share']:.5f} (cap {rc.MAX_EXCLUDED_SHARE}), mirrored crops checked whole {mirror_checked}")
    assert worst["share"] <= rc.MAX_EXCLUDED_SHARE
    assert worst["tri"] == 0 and worst["bg"] == 0
    assert worst["depth"] <= rc.EPS_MM and worst["shade"] <= 1
    assert mirror_checked > 0


def test_batch_independence_and_determinism(scene):
    m, v, cp, sr = scene["mesh"], scene["verts"], scene["crop_params"], scene["sample_range"]
    again = _native.render_mesh(m, v, cp, sr)
    assert all(torch.equal(a, b) for a, b in zip(again, (scene["depth"], scene["tri"], scene["shade"])))
    half = 369
    n_half = int(sr[half - 1, 1])
    part = _native.render_mesh(m, v[:half].contiguous(), cp[:n_half].contiguous(), sr[:half].contiguous())
    assert torch.equal(part[0], scene["depth"][:n_half]) and torch.equal(part[1], scene["tri"][:n_half]) and torch.equal(part[2], scene["shade"][:n_half])
    for i in (0, 200, 737):
        c0, c1 = int(sr[i, 0]), int(sr[i, 1])
        one = _native.render_mesh(m, v[i:i + 1].contiguous(), cp[c0:c1].contiguous(), torch.tensor([[0, c1 - c0]], device=DEV))
        assert torch.equal(one[0], scene["depth"][c0:c1]) and torch.equal(one[1], scene["tri"][c0:c1]) and torch.equal(one[2], scene["shade"][c0:c1])


def test_edge_cases(scene):
    m, v, cp, sr = scene["mesh"], scene["verts"], scene["crop_params"], scene["sample_range"]
    c0 = int(sr[3, 0])
    assert int(sr[3, 1]) - c0 == 2
    # one view writes one crop, zero views write nothing
    d = torch.full((3, 96, 96), -7.0, device=DEV)
    t = torch.full((3, 96, 96), -7, dtype=torch.int32, device=DEV)
    s = torch.full((3, 96, 96), 7, dtype=torch.uint8, device=DEV)
    _native.render_mesh(m, v[3:5].contiguous(), cp[c0:c0 + 3].contiguous(), torch.tensor([[1, 2], [2, 2]], device=DEV), depth=d, tri=t, shade=s)
    assert (d[0] == -7).all() and (d[2] == -7).all() and (t[0] == -7).all() and (t[2] == -7).all() and (s[0] == 7).all() and (s[2] == 7).all()
    assert torch.equal(t[1], scene["tri"][c0 + 1]) and torch.equal(d[1], scene["depth"][c0 + 1]) and torch.equal(s[1], scene["shade"][c0 + 1])
    # optional outputs
    only = _native.render_mesh(m, v[3:4].contiguous(), cp[c0:c0 + 2].contiguous(), torch.tensor([[0, 2]], device=DEV), depth=False, shade=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], scene["tri"][c0:c0 + 2])
    # vertices behind the camera: their triangles are skipped, nothing is reported
    row = cp[c0].cpu().numpy()
    vb = v[3:4].clone()
    eye_z = rc.project(vb[0].cpu().numpy(), row)[0][:, 2]
    far = int(np.argmax(eye_z))
    cam_pos = torch.from_numpy(row[13:16]).to(DEV, torch.float32)
    vb[0, far] = cam_pos - (vb[0, far] - cam_pos)                    # mirrored through the eye: behind it
    got = _native.render_mesh(m, vb, cp[c0:c0 + 1].contiguous(), torch.tensor([[0, 1]], device=DEV))
    y = rc.rasterise(vb[0].cpu().numpy(), scene["triangles"], row, delta=rc.DELTA_PX, eps=rc.EPS_MM)
    uses = (scene["triangles"] == far).any(1)
    assert uses.any() and not np.isin(got[1].cpu().numpy(), np.nonzero(uses)[0]).any()
    ok = ~y["excluded"]
    assert np.array_equal(got[1][0].cpu().numpy()[ok], y["tri"][ok])
    # a bad sample_range: IndexError, nothing drawn; deferred on an engine: status bit at the next poll
    for bad in ([[0, 3]], [[-1, 1]], [[2, 1]], [[0, 4]]):
        d.fill_(-7.0)
        with pytest.raises(IndexError, match="ut_render_mesh"):
            _native.render_mesh(m, v[3:4].contiguous(), cp[c0:c0 + 3].contiguous(), torch.tensor(bad, device=DEV), depth=d, tri=t, shade=s)
        assert (d == -7).all()
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with eng.modes(deferred_checks=True):
            t.fill_(-7)
            _native.render_mesh(m, v[3:5].contiguous(), cp[c0:c0 + 3].contiguous(), torch.tensor([[0, 1], [1, 5]], device=DEV), depth=d, tri=t, shade=s, engine=eng)
            torch.cuda.synchronize()
            assert (t == -7).all()                                       # the good row is not drawn either
            with pytest.raises(IndexError, match="sample_range"):
                eng.poll_status()
            _native.render_mesh(m, v[3:4].contiguous(), cp[c0:c0 + 3].contiguous(), torch.tensor([[0, 2]], device=DEV), depth=d, tri=t, shade=s, engine=eng)
            eng.poll_status()
            assert torch.equal(t[:2], scene["tri"][c0:c0 + 2])
    finally:
        eng.close()
    # refusals
    with pytest.raises(ValueError, match="crop_size must be 96"):
        _native.render_mesh(m, v[3:4].contiguous(), cp[c0:c0 + 1].contiguous(), torch.tensor([[0, 1]], device=DEV), crop_size=64)
    vv, _, ww = mc.load_mesh("rec00")
    with pytest.raises(ValueError, match="no triangles"):
        bare = _native.Mesh(vv, np.zeros((0, 3), np.int32), ww, DEV)
        _native.render_mesh(bare, v[3:4].contiguous(), cp[c0:c0 + 1].contiguous(), torch.tensor([[0, 1]], device=DEV))


def test_python_surface(scene, labels, hm_t):
    i = 41
    f, h = divmod(i, 2)
    pose = tracker.SingleHandPose(joint_angles=labels["joint_angles"][f, h], wrist_xform=labels["wrist_transforms"][f, h])
    sr = scene["sample_range"].cpu().numpy()
    assert scene["hand"][i] == h
    cams = [tracker._crop_camera_from_row(r, None, None, 96) for r in scene["crop_params"][sr[i, 0]:sr[i, 1]].cpu().numpy()]
    depth, tri, shade = tracker.render_hand_pose(hm_t, pose, h, dict(enumerate(cams)))
    assert depth.shape == (len(cams), 96, 96) and tri.dtype == np.int32 and shade.dtype == np.uint8
    assert np.array_equal(tri, scene["tri"][sr[i, 0]:sr[i, 1]].cpu().numpy())
    assert np.array_equal(depth, scene["depth"][sr[i, 0]:sr[i, 1]].cpu().numpy())
    from lib.common.hand_skinning import overlay, render_mesh as dropin
    assert dropin is hand.render_mesh and overlay is hand.overlay
    crops = torch.rand(len(cams), 96, 96)
    mixed = hand.overlay(crops, torch.from_numpy(shade), torch.from_numpy(tri), alpha=0.5)
    bg = torch.from_numpy(tri) < 0
    assert torch.equal(mixed[bg], crops[bg]) and not torch.equal(mixed[~bg], crops[~bg]) and bool(bg.any()) and bool((~bg).any())


@pytest.mark.timeout(240, method="thread")
def test_hot_path_with_render(labels, hm_t):
    """HotPath(render=True): the records are those of a plain HotPath, the render buffers are ut_render_mesh of the step's
    vertices, and the whole step - render included - replays four times from one hipGraph with the eager step's bits."""
    frames = 24
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        src_a = torch.randint(0, 256, (frames * 4, 480, 636), dtype=torch.uint8, device=DEV, generator=g)
        src_b = torch.randint(0, 256, (frames * 4, 480, 636), dtype=torch.uint8, device=DEV, generator=g)
        plan = {k: v.cpu().numpy() for k, v in pipeline.crop_plan_on_device(labels, hm_t, range(frames), DEV).items()}
        batch = pipeline.make_batch(plan, src_a.clone(), DEV)
        plain = pipeline.HotPath(eng, hm_t).step(batch).clone()
        hot = pipeline.HotPath(eng, hm_t, render=True)
        assert hot.mesh is not None
        want_a = hot.step(batch).clone()
        assert torch.equal(want_a, plain)
        ra = tuple(x.clone() for x in (hot.render_depth, hot.render_tri, hot.render_shade))
        assert tuple(ra[0].shape) == (batch.n_crops, 96, 96)
        direct = _native.render_mesh(hot.mesh, hot.mesh_vertices, batch.crop_params, batch.sample_range)
        assert all(torch.equal(a, b) for a, b in zip(direct, ra))
        batch.src.copy_(src_b)
        want_b = hot.step(batch).clone()
        rb = tuple(x.clone() for x in (hot.render_depth, hot.render_tri, hot.render_shade))
        hot.check()
        assert not torch.equal(ra[0], rb[0])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                rec = hot.step(batch)
        for inp, want, rr in ((src_a, want_a, ra), (src_b, want_b, rb), (src_a, want_a, ra), (src_b, want_b, rb)):
            batch.src.copy_(inp)
            rec.zero_()
            hot.render_depth.zero_(); hot.render_tri.zero_(); hot.render_shade.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(rec, want)
            assert torch.equal(hot.render_depth, rr[0]) and torch.equal(hot.render_tri, rr[1]) and torch.equal(hot.render_shade, rr[2])
        hot.check()
        del graph
    finally:
        eng.close()
