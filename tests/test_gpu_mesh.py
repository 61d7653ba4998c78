"""GPU tests of the posed hand mesh (csrc/mesh.hip through ut_mesh_create / ut_skin_mesh) against the float64 oracle of
tests/mesh_cases.py, which tests/test_mesh_host.py pins to the landmark oracle.

Bounds: vertices 1e-3 mm (the project's keypoint tolerance); normals 4 x the distance of the numpy float32 restatement
to float64 on the same poses, computed here (the margin covers another cross / sum order and the device's sin / cos /
sqrt)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_cases as mc
from absolutetrack_amd import _native, arch, hand, pipeline, synth, tracker

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VERTEX_TOL_MM = 1e-3


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _blob(hm):
    return _t(_native.hand_model_blob(hm["joint_rotation_axes"], hm["joint_rest_positions"], hm["landmark_rest_positions"],
                                      hm["landmark_rest_bone_weights"], hm["landmark_rest_bone_indices"])).reshape(-1, 321)


def _skin(mesh, blob, ja, xf, mirror=None, normals=False, t_scale=1.0):
    res = _native.skin_mesh(mesh, blob, _t(ja), _t(xf), mirror=None if mirror is None else _t(mirror, torch.int64),
                            t_scale=t_scale, normals=normals)
    torch.cuda.synchronize()
    return (res[0].cpu().numpy(), res[1].cpu().numpy()) if normals else res.cpu().numpy()


@pytest.fixture(scope="module")
def labels():
    return pipeline.load_labels()


@pytest.fixture(scope="module")
def hm(labels):
    return mc.skeleton(np.load(pipeline._DATA), "hm.")


@pytest.fixture(scope="module")
def rec00(hm, labels):
    """The recording's mesh, all 369 x 2 label poses (right hands through the mirror flag), both oracles."""
    v, t, w = mc.load_mesh("rec00")
    ja, xf, hand_idx = mc.label_poses(labels)
    p64, n64 = mc.skin(hm, v, w, ja.astype(np.float32), xf.astype(np.float32), triangles=t, dtype=np.float64, mirror=hand_idx)
    p32, n32 = mc.skin(hm, v, w, ja.astype(np.float32), xf.astype(np.float32), triangles=t, dtype=np.float32, mirror=hand_idx)
    mesh = _native.Mesh(v, t, w, DEV)
    got_p, got_n = _skin(mesh, _blob(hm), ja, xf, mirror=hand_idx, normals=True)
    return dict(v=v, t=t, w=w, ja=ja, xf=xf, hand=hand_idx, p64=p64, n64=n64, p32=p32, n32=n32, mesh=mesh, got_p=got_p,
                got_n=got_n)


def test_vertices_match_float64_oracle(rec00, hm):
    assert rec00["mesh"].counts() == (788, 1544) and rec00["got_p"].shape == (738, 788, 3)
    err = np.abs(rec00["got_p"] - rec00["p64"]).max()
    yard = np.abs(rec00["p32"] - rec00["p64"]).max()
    print(f"recording mesh, 738 poses: GPU vs float64 {err:.3e} mm (numpy float32 vs float64 {yard:.3e} mm, |coordinate| <= "
          f"{np.abs(rec00['p64']).max():.0f} mm)")
    assert err <= VERTEX_TOL_MM
    # vertices alone (no normal output) are the same bits
    only = _skin(rec00["mesh"], _blob(hm), rec00["ja"], rec00["xf"], mirror=rec00["hand"])
    assert np.array_equal(only, rec00["got_p"])
    # the generic mesh on a subset of the poses
    v, t, w = mc.load_mesh("generic")
    sub = slice(0, 738, 7)
    want = mc.skin(hm, v, w, rec00["ja"][sub].astype(np.float32), rec00["xf"][sub].astype(np.float32), mirror=rec00["hand"][sub])
    got = _skin(_native.Mesh(v, t, w, DEV), _blob(hm), rec00["ja"][sub], rec00["xf"][sub], mirror=rec00["hand"][sub])
    err_g = np.abs(got - want).max()
    print(f"generic mesh, {want.shape[0]} poses: GPU vs float64 {err_g:.3e} mm")
    assert err_g <= VERTEX_TOL_MM
    assert np.abs(got - rec00["got_p"][sub]).max() > 1.0          # really another mesh


def test_normals_match_float64_oracle(rec00):
    yard = np.abs(rec00["n32"].astype(np.float64) - rec00["n64"]).max()
    err = np.abs(rec00["got_n"].astype(np.float64) - rec00["n64"]).max()
    length = np.linalg.norm(rec00["got_n"].astype(np.float64), axis=-1)
    print(f"normals, 738 poses: GPU vs float64 {err:.3e} per component; yardstick (numpy float32 vs float64) {yard:.3e}; "
          f"bound {4 * yard:.3e}; |n| in [{length.min():.7f}, {length.max():.7f}]")
    assert 0 < yard < 1e-3
    assert err <= 4 * yard
    assert np.abs(length - 1).max() <= 1e-5


def test_landmarks_through_the_mesh_path(golden_dir):
    """A 'mesh' of the 21 landmark rest positions with densified landmark weights is ut_fk: both kernels build their
    frames with the same code and blend in ascending frame order.  Bit-for-bit equality does NOT hold (measured on MI355X):
    the compiler contracts the 4-slot blend of mesh.hip and the 17-frame blend of fk.hip into different multiply-add
    chains, so single coordinates differ in the last place.  Asserted: at most one unit in the last place of the largest
    coordinate.  The result is also within 1e-3 mm of the keypoints the reference stored (gt_keypoints)."""
    g = np.load(os.path.join(golden_dir, "fk_user05.npz"))
    n_checked, all_equal, worst = 0, True, 0.0
    for rec in ("00", "02", "11"):
        p = f"r{rec}."
        hmr = mc.skeleton(g, p + "hm.")
        mesh = _native.Mesh(hmr["landmark_rest_positions"], np.zeros((0, 3), np.int32), mc.dense_landmark_weights(hmr), DEV)
        assert mesh.counts() == (21, 0)
        for hand_idx in (0, 1):
            ja, xf = g[p + "joint_angles"][:, hand_idx], g[p + "wrist_transforms"][:, hand_idx]
            mirror = np.full(len(ja), hand_idx)
            got, nrm = _skin(mesh, _blob(hmr), ja, xf, mirror=mirror, normals=True)
            fk = _native.fk_stateless(_blob(hmr), _t(ja), _t(xf), mirror=_t(mirror, torch.int64)).cpu().numpy()
            ulp = np.spacing(np.float32(np.abs(fk).max()))
            diff = np.abs(got - fk).max()
            worst = max(worst, float(diff))
            all_equal &= bool(np.array_equal(got, fk))
            assert diff <= ulp, (rec, hand_idx, diff, ulp)
            assert np.array_equal(nrm, np.zeros_like(nrm))           # no triangles: zero normals
            valid = g[p + "valid_tracking"][hand_idx]
            err = np.abs(got - g[p + "gt_keypoints"][hand_idx])[valid]
            assert err.max() < 1e-3, (rec, hand_idx, err.max())
            n_checked += int(valid.sum())
    print(f"landmarks through ut_skin_mesh vs ut_fk: bit-equal = {all_equal}, largest difference {worst:.3e} mm")
    assert n_checked > 250


def test_right_hands(rec00, hm):
    right = rec00["hand"] == 1
    ja, xf = rec00["ja"][right], rec00["xf"][right]
    flipped = xf.copy()
    flipped[:, :, 0] *= -1
    want_p, want_n = mc.skin(hm, rec00["v"], rec00["w"], ja.astype(np.float32), flipped.astype(np.float32), triangles=rec00["t"])
    got_p, got_n = rec00["got_p"][right], rec00["got_n"][right]
    yard = np.abs(rec00["n32"].astype(np.float64) - rec00["n64"]).max()
    assert np.abs(got_p - want_p).max() <= VERTEX_TOL_MM
    assert np.abs(got_n.astype(np.float64) + want_n).max() <= 4 * yard        # the oracle's normal with the sign flipped
    # the device's negation is the host's: the mirrored call equals the unmirrored call on the negated transform
    host = _skin(rec00["mesh"], _blob(hm), ja, flipped)
    assert np.array_equal(host, got_p)
    # a reflected mesh has its winding reversed: positive volume with the triangles read backwards, and for left hands as stored
    assert (mc.signed_volume(got_p, rec00["t"][:, ::-1]) > 1e5).all()
    assert (mc.signed_volume(rec00["got_p"][~right], rec00["t"]) > 1e5).all()
    # normals point outwards on both hands: stepping along them grows the enclosed volume
    for sel, tri in ((right, rec00["t"][:, ::-1]), (~right, rec00["t"])):
        p, nrm = rec00["got_p"][sel][:40].astype(np.float64), rec00["got_n"][sel][:40].astype(np.float64)
        assert (mc.signed_volume(p + nrm, tri) > mc.signed_volume(p, tri)).all()


def test_call_shape_invariances(rec00, hm):
    mesh, blob = rec00["mesh"], _blob(hm)
    ja, xf, hand_idx = rec00["ja"], rec00["xf"], rec00["hand"]
    # ---- pose records in place (row stride 60) against contiguous copies
    n = 300
    rec = torch.zeros(n, arch.POSE_REC, device=DEV)
    rec[:, :22] = _t(ja[:n])
    rec[:, 22:38] = _t(xf[:n]).reshape(n, 16)
    mirror = _t(hand_idx[:n], torch.int64)
    pv, pn = _native.skin_mesh(mesh, blob, rec, rec[:, 22:], mirror=mirror, normals=True, ja_stride=arch.POSE_REC,
                               xf_stride=arch.POSE_REC, n=n)
    assert torch.equal(pv.cpu(), torch.from_numpy(rec00["got_p"][:n])) and torch.equal(pn.cpu(), torch.from_numpy(rec00["got_n"][:n]))
    # ---- metres with t_scale 1000 against mm with t_scale 1
    xf_m = xf[:n].copy()
    xf_m[:, :3, 3] *= 0.001
    got_m = _skin(mesh, blob, ja[:n], xf_m, mirror=hand_idx[:n], t_scale=1000.0)
    d = np.abs(got_m - rec00["got_p"][:n]).max()
    print(f"t_scale 1000 on metres vs 1 on mm: {d:.3e} mm")
    assert d <= 1e-3
    # ---- one skeleton per pose against the loop over single calls
    k = 12
    scales = np.linspace(0.8, 1.25, k).astype(np.float32)
    per_pose = {"joint_rotation_axes": np.broadcast_to(hm["joint_rotation_axes"], (k, 22, 3)),
                "joint_rest_positions": hm["joint_rest_positions"][None] * scales[:, None, None],
                "landmark_rest_positions": hm["landmark_rest_positions"][None] * scales[:, None, None],
                "landmark_rest_bone_weights": hm["landmark_rest_bone_weights"], "landmark_rest_bone_indices": hm["landmark_rest_bone_indices"]}
    blobs = _blob(per_pose)
    assert blobs.shape == (k, 321)
    bv, bn = _skin(mesh, blobs, ja[:k], xf[:k], mirror=hand_idx[:k], normals=True)
    for i in range(k):
        sv, sn = _skin(mesh, blobs[i:i + 1].contiguous(), ja[i:i + 1], xf[i:i + 1], mirror=hand_idx[i:i + 1], normals=True)
        assert np.array_equal(sv[0], bv[i]) and np.array_equal(sn[0], bn[i])
    assert np.abs(bv[0] - rec00["got_p"][0]).max() > 0.1           # the skeleton really is per pose
    # ---- a pose's result does not depend on its batch
    idx = np.arange(2048) % 738
    big_v, big_n = _skin(mesh, blob, ja[idx], xf[idx], mirror=hand_idx[idx], normals=True)
    assert np.array_equal(big_v, rec00["got_p"][idx]) and np.array_equal(big_n, rec00["got_n"][idx])
    v13, n13 = _skin(mesh, blob, ja[idx[:13]], xf[idx[:13]], mirror=hand_idx[idx[:13]], normals=True)
    assert np.array_equal(v13, big_v[:13]) and np.array_equal(n13, big_n[:13])
    for i in (0, 12, 2047):
        v1, n1 = _skin(mesh, blob, ja[idx[i:i + 1]], xf[idx[i:i + 1]], mirror=hand_idx[idx[i:i + 1]], normals=True)
        assert np.array_equal(v1[0], big_v[i]) and np.array_equal(n1[0], big_n[i])
    # ---- n = 0
    lib = _native.load_library()
    assert lib.ut_skin_mesh(None, mesh._h, None, 1, None, 22, None, 16, None, ctypes.c_float(1.0), 0, None, None, None) == 0
    empty = _native.skin_mesh(mesh, blob, torch.zeros(0, 22, device=DEV), torch.zeros(0, 4, 4, device=DEV))
    assert tuple(empty.shape) == (0, 788, 3)


def test_rejections_leave_the_device_usable(rec00, hm):
    lib = _native.load_library()
    v, t, w = rec00["v"], rec00["t"], rec00["w"]

    def refused(v, t, w, code, words):
        h = ctypes.c_void_p()
        rc = lib.ut_mesh_create(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], w.ctypes.data, 0, ctypes.byref(h))
        msg = lib.ut_last_error(None).decode()
        assert rc == code and not h.value and words in msg, (rc, msg)
        with pytest.raises(ValueError, match="ut_mesh_create"):
            _native.Mesh(v, t, w, DEV)
        # the device and the library still work: a valid mesh and a valid launch afterwards
        got = _skin(_native.Mesh(rec00["v"], rec00["t"], rec00["w"], DEV), _blob(hm), rec00["ja"][:3], rec00["xf"][:3],
                    mirror=rec00["hand"][:3])
        assert np.array_equal(got, rec00["got_p"][:3])

    bad = w.copy(); bad[5, :5] = 0.2
    refused(v, t, bad, -4, "vertex 5 has more than 4 non-zero bone weights")
    bad = t.copy(); bad[7, 1] = v.shape[0]
    refused(v, bad, w, -1, "triangle 7 names vertex 788")
    bad = w.copy(); bad[3, 0] = np.nan
    refused(v, t, bad, -1, "weight [3][0] is not finite")
    nv = 5056 + 1
    refused(np.zeros((nv, 3), np.float32), t, np.tile(w[:1], (nv, 1)), -4, "UT_MESH_MAX_VERTICES")
    refused(v[:0], t[:0], w[:0], -1, "no vertices")
    # bad launch arguments are refused before anything is enqueued
    mesh, blob = rec00["mesh"], _blob(hm)
    ja, xf = _t(rec00["ja"][:4]), _t(rec00["xf"][:4])
    out = torch.empty(4, 788, 3, device=DEV)
    rc = lib.ut_skin_mesh(None, mesh._h, blob.data_ptr(), 3, ja.data_ptr(), 22, xf.data_ptr(), 16, None, ctypes.c_float(1.0), 4,
                          out.data_ptr(), None, None)
    assert rc == -1 and "ut_skin_mesh" in lib.ut_last_error(None).decode()
    rc = lib.ut_skin_mesh(None, None, blob.data_ptr(), 1, ja.data_ptr(), 22, xf.data_ptr(), 16, None, ctypes.c_float(1.0), 4,
                          out.data_ptr(), None, None)
    assert rc == -1 and "null mesh" in lib.ut_last_error(None).decode()


def test_largest_supported_mesh(hm, rec00):
    """UT_MESH_MAX_VERTICES vertices (the whole LDS budget of a workgroup), four influences each, an odd vertex count too
    (the scalar store path): against the float64 oracle."""
    rng = np.random.default_rng(7)
    for nv in (5056, 1001):
        v = rng.uniform(-100, 100, (nv, 3)).astype(np.float32)
        w = np.zeros((nv, 17), np.float32)
        for i in range(nv):
            w[i, rng.choice(17, 4, replace=False)] = rng.dirichlet(np.ones(4)).astype(np.float32) + np.float32(0.01)
        t = rng.integers(0, nv, (2 * nv, 3)).astype(np.int32)
        t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
        ja, xf, hand_idx = rec00["ja"][:6], rec00["xf"][:6], rec00["hand"][:6]
        want = mc.skin(hm, v, w, ja.astype(np.float32), xf.astype(np.float32), mirror=hand_idx)
        mesh = _native.Mesh(v, t, w, DEV)
        got, nrm = _skin(mesh, _blob(hm), ja, xf, mirror=hand_idx, normals=True)
        err = np.abs(got - want).max()
        print(f"{nv} random vertices, 4 influences: GPU vs float64 {err:.3e} mm")
        assert err <= VERTEX_TOL_MM
        used = np.zeros(nv, bool)
        used[t.reshape(-1)] = True
        length = np.linalg.norm(nrm.astype(np.float64), axis=-1)
        assert np.abs(length[:, used] - 1).max() <= 1e-5 and (length[:, ~used] == 0).all()


def _mesh_hand_model(labels):
    v, t, w = mc.load_mesh("rec00")
    return pipeline.hand_model_from_labels(labels)._replace(mesh_vertices=torch.from_numpy(v), mesh_triangles=torch.from_numpy(t),
                                                            dense_bone_weights=torch.from_numpy(w))


@pytest.mark.timeout(240, method="thread")
@pytest.mark.parametrize("conv,frames", [("fp32", 24), ("split_f16", 300)])
def test_hot_path_with_mesh(labels, conv, frames):
    """HotPath(mesh=True, mesh_normals=True): the records are those of a HotPath without a mesh, the mesh is ut_skin_mesh of the
    step's records, and the whole step - mesh included - replays from one hipGraph with the eager step's bits."""
    hm_t = _mesh_hand_model(labels)
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        with pytest.raises(ValueError, match="no mesh"):
            pipeline.HotPath(eng, pipeline.hand_model_from_labels(labels), mesh=True)
        eng.set_conv_arithmetic(conv)
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        src_a = torch.randint(0, 256, (frames * 4, 480, 636), dtype=torch.uint8, device=DEV, generator=g)
        src_b = torch.randint(0, 256, (frames * 4, 480, 636), dtype=torch.uint8, device=DEV, generator=g)
        plan = {k: v.cpu().numpy() for k, v in pipeline.crop_plan_on_device(labels, hm_t, range(frames), DEV).items()}
        batch = pipeline.make_batch(plan, src_a.clone(), DEV)
        plain = pipeline.HotPath(eng, hm_t).step(batch).clone()
        hot = pipeline.HotPath(eng, hm_t, mesh=True, mesh_normals=True)
        want_a = hot.step(batch).clone()
        assert torch.equal(want_a, plain)
        s = batch.n_samples
        assert tuple(hot.mesh_vertices.shape) == (s, 788, 3) and tuple(hot.mesh_normals.shape) == (s, 788, 3)
        mesh_a, nrm_a = hot.mesh_vertices.clone(), hot.mesh_normals.clone()
        sv, sn = _native.skin_mesh(hot.mesh, hot.hand_blob, want_a[:, :22].contiguous(), want_a[:, 22:38].contiguous(),
                                   mirror=batch.hand_idx, t_scale=1000.0, normals=True)
        assert torch.equal(sv, mesh_a) and torch.equal(sn, nrm_a)
        assert torch.isfinite(mesh_a).all() and (nrm_a.norm(dim=-1) - 1).abs().max() <= 1e-5
        batch.src.copy_(src_b)
        want_b = hot.step(batch).clone()
        mesh_b, nrm_b = hot.mesh_vertices.clone(), hot.mesh_normals.clone()
        hot.check()
        assert not torch.equal(mesh_a, mesh_b)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                rec = hot.step(batch)
        for inp, want, mv, mn in ((src_a, want_a, mesh_a, nrm_a), (src_b, want_b, mesh_b, nrm_b), (src_a, want_a, mesh_a, nrm_a)):
            batch.src.copy_(inp)
            rec.zero_()
            hot.mesh_vertices.zero_()
            hot.mesh_normals.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(rec, want) and torch.equal(hot.mesh_vertices, mv) and torch.equal(hot.mesh_normals, mn)
        hot.check()
        del graph
    finally:
        eng.close()


def test_python_surface(labels, rec00, hm):
    hm_t = _mesh_hand_model(labels)
    ja = torch.from_numpy(rec00["ja"][:12]).float().reshape(3, 4, 22)
    xf = torch.from_numpy(rec00["xf"][:12]).float().reshape(3, 4, 4, 4)
    mirror = torch.from_numpy(rec00["hand"][:12]).reshape(3, 4)
    v, n = hand.skin_mesh(hm_t, ja, xf, normals=True, mirror=mirror)
    assert tuple(v.shape) == (3, 4, 788, 3) and tuple(n.shape) == (3, 4, 788, 3) and v.device.type == "cpu"
    assert np.array_equal(v.reshape(12, 788, 3).numpy(), rec00["got_p"][:12])
    assert np.array_equal(n.reshape(12, 788, 3).numpy(), rec00["got_n"][:12])
    only = hand.skin_mesh(hm_t, ja.to(DEV), xf.to(DEV), mirror=mirror)
    assert only.device.type == "cuda" and torch.equal(only.cpu(), v)
    assert hand.device_mesh(hm_t, torch.device(DEV)) is hand.device_mesh(hm_t, torch.device(DEV))       # packed once
    from lib.common.hand_skinning import skin_mesh as dropin
    assert dropin is hand.skin_mesh
    # unbatched pose, batched skeleton
    one = hand.skin_mesh(hm_t, ja[0, 0], xf[0, 0])
    assert tuple(one.shape) == (788, 3) and np.abs(one.numpy() - mc.skin(hm, rec00["v"], rec00["w"], rec00["ja"][:1].astype(np.float32),
                                                                          rec00["xf"][:1].astype(np.float32))[0]).max() <= VERTEX_TOL_MM
    batched = hm_t._replace(joint_rest_positions=hm_t.joint_rest_positions.expand(3, 4, 22, 3).clone(),
                            joint_rotation_axes=hm_t.joint_rotation_axes.expand(3, 4, 22, 3).clone())
    assert torch.equal(hand.skin_mesh(batched, ja, xf, mirror=mirror), v)
    with pytest.raises(ValueError, match="no mesh"):
        hand.skin_mesh(pipeline.hand_model_from_labels(labels), ja, xf)
    with pytest.raises(ValueError, match="unbatched"):
        hand.skin_mesh(hm_t._replace(mesh_vertices=hm_t.mesh_vertices.expand(3, 4, 788, 3)), ja, xf)
    # mesh_from_hand_pose: the mesh twin of landmarks_from_hand_pose
    pose = tracker.SingleHandPose(joint_angles=labels["joint_angles"][40, 1], wrist_xform=labels["wrist_transforms"][40, 1])
    mv, mn = tracker.mesh_from_hand_pose(hm_t, pose, 1, normals=True)
    lv, ln = hand.skin_mesh(hm_t, torch.from_numpy(pose.joint_angles).float(),
                            torch.from_numpy(tracker._left_handed(pose.wrist_xform, 1)).float(), normals=True)
    assert mv.shape == (788, 3) and np.array_equal(mv, lv.numpy())
    assert np.array_equal(mn, -ln.numpy())         # same surface; the flag keeps the right hand's normals pointing outwards
    assert np.array_equal(tracker.mesh_from_hand_pose(hm_t, pose._replace(wrist_xform=labels["wrist_transforms"][40, 0]), 0),
                          hand.skin_mesh(hm_t, torch.from_numpy(pose.joint_angles).float(),
                                         torch.from_numpy(labels["wrist_transforms"][40, 0]).float()).numpy())
