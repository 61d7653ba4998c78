"""CPU tests of the rendered hand: the C declarations, the host refusals of ut_project_points / ut_render_mesh, the float64
yardstick rasteriser of tests/render_cases.py against an image worked out by hand, the yardstick's own excluded share and the
constants DELTA_PX / EPS_MM against a re-measurement, and the host path of project_landmarks against the reference's numbers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import render_cases as rc
from absolutetrack_amd import geometry, pipeline, tracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_render_entries_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "render_c99.c"), "-o", str(tmp_path / "render_c99.o")])


def test_library_exports_the_entries_and_refuses_on_the_host():
    """Argument validation happens before any device is touched, so the refusals can be checked here; ut_mesh_create still
    refuses what it refused."""
    from absolutetrack_amd import _native
    lib = _native.load_library()
    for name in ("ut_project_points", "ut_render_mesh"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    v, t, w = mc.load_mesh("rec00")
    h = ctypes.c_void_p()
    bad = t.copy(); bad[7, 1] = v.shape[0]
    assert lib.ut_mesh_create(v.ctypes.data, v.shape[0], bad.ctypes.data, bad.shape[0], w.ctypes.data, 0, ctypes.byref(h)) == -1
    assert "triangle 7 names vertex 788" in lib.ut_last_error(None).decode() and not h.value
    bad = w.copy(); bad[5, :5] = 0.2
    assert lib.ut_mesh_create(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], bad.ctypes.data, 0, ctypes.byref(h)) == -4
    assert lib.ut_last_error(None).decode() == "ut_mesh_create: vertex 5 has more than 4 non-zero bone weights"

    def err(rc_):
        return rc_, lib.ut_last_error(None).decode()
    assert err(lib.ut_render_mesh(None, None, None, None, 0, None, 1, 96, None, None, None, None)) == (-1, "ut_render_mesh: null mesh")
    buf = np.zeros(64)
    p, i32p = buf.ctypes.data, buf.ctypes.data
    rc_, msg = err(lib.ut_project_points(None, None, 63, 21, i32p, 1, p, 1, 0, 1, 640, 480, p, p, p, None))
    assert rc_ == -1 and msg == "ut_project_points: null argument"
    rc_, msg = err(lib.ut_project_points(None, ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), 63, 21, i32p, 1, p, 1, 7, 1, 640, 480, p, p, p, None))
    assert rc_ == -1 and "table_kind" in msg
    rc_, msg = err(lib.ut_project_points(None, ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), 62, 21, i32p, 1, p, 1, 0, 1, 640, 480, p, p, p, None))
    assert rc_ == -1 and msg == "ut_project_points: bad argument"


def test_yardstick_reproduces_a_hand_computed_image():
    """rc.hand_case(): f = 128, c = 0, camera at the origin.
    Triangle 0, z = 128: screen (0,0) (8,0) (0,8).  Top edge y = 0 and left edge x = 0 count, the hypotenuse x + y = 8 does not
    (neither top nor left): pixels x, y >= 0, x + y <= 7 -> 8 + 7 + .. + 1 = 36.
    Triangle 1: (1,1,64) -> (2,2), (10,2,128) -> (10,2), (1,5,64) -> (2,10): pixels x, y >= 2, (x-2) + (y-2) <= 7 -> 36.
    Overlap: x, y >= 2 and x + y <= 7 -> 4 + 3 + 2 + 1 = 10 pixels; there triangle 1 is nearer (its z < 128 away from its
    vertex (10,2), which lies outside triangle 0), so triangle 0 keeps 26 and 62 pixels are covered.
    Depth: 1 / z is linear on the screen.  (0,0): triangle 0, z = 128.  (6,2): half way from (2,2) to (10,2),
    1 / z = (1/64 + 1/128) / 2 = 3/256, z = 256/3 (not the 96 of linear z).  (4,4): a quarter of the way towards (10,2),
    none towards (2,10): 1 / z = 1/64 - (1/4)(1/64 - 1/128) = 7/512, z = 512/7.
    Triangle 2 has a vertex at z = -10: skipped whole, though its other vertices would cover much of the image.
    Triangle 3 is triangle 0 again: equal depth, the lower index wins everywhere.
    Shade of triangle 0: n = (0,0,1), centroid (8/3, 8/3, 128): cos = 128 / sqrt(128^2 + 2 (8/3)^2) = 0.99978 -> 255."""
    v, t, row = rc.hand_case()
    r = rc.rasterise(v, t, row)
    assert r["covered"] == 62 and (r["tri"] >= 0).sum() == 62
    assert (r["tri"] == 0).sum() == 26 and (r["tri"] == 1).sum() == 36 and (r["tri"] == 2).sum() == 0 and (r["tri"] == 3).sum() == 0
    ys, xs = np.nonzero(r["tri"] == 1)
    assert set(zip(xs.tolist(), ys.tolist())) == {(x, y) for x in range(2, 10) for y in range(2, 10) if x + y <= 11}
    assert r["tri"][0, 7] == 0 and r["tri"][0, 8] == -1 and r["tri"][4, 4] == 1 and r["tri"][1, 6] == 0 and r["tri"][7, 0] == 0
    assert r["depth"][0, 0] == 128.0
    assert abs(r["depth"][2, 6] - 256.0 / 3.0) < 1e-12 and abs(r["depth"][4, 4] - 512.0 / 7.0) < 1e-12
    assert r["depth2"][4, 3] == 128.0 and np.isinf(r["depth2"][2, 9]) and np.isinf(r["depth"][50, 50])
    assert r["shade"][0, 0] == 255 and r["shade"][50, 50] == 0
    # the float32 restatement draws the same picture
    r32 = rc.rasterise(v, t, row, np.float32)
    assert np.array_equal(r32["tri"], r["tri"]) and np.abs(r32["depth"][r["tri"] >= 0] - r["depth"][r["tri"] >= 0]).max() < 1e-4
    # mirrored camera (diag(-1,1,1) world->eye, the crop camera of a right hand): the picture flips in x, nothing else changes
    row_m = row.copy()
    row_m[4:13] = np.diag([-1.0, 1.0, 1.0]).reshape(-1)
    row_m[2] = 20.0
    m = rc.rasterise(v, t, row_m)
    assert m["covered"] == 62 + 0 and m["tri"][4, 16] == 1 and m["shade"][0, 19] == 255 and m["tri"][0, 20] == -1   # x = 20 is a right edge now


@pytest.fixture(scope="module")
def sampled():
    """Every 9th label pose of recording_00 (82 poses, their one or two crop cameras from the host oracle), float32 vertices
    from the float32 mesh oracle: float32-vs-float64 disagreement and the excluded share per crop."""
    lab = pipeline.load_labels()
    hm = mc.skeleton(np.load(pipeline._DATA), "hm.")
    v, t, w = mc.load_mesh("rec00")
    ja, xf, hand = mc.label_poses(lab)
    edge = depth = 0.0
    shares, covered = [], []
    for pid, rows in rc.label_crops_host(lab, hm, range(0, 738, 9)):
        p = mc.skin(hm, v, w, ja[pid:pid + 1].astype(np.float32), xf[pid:pid + 1].astype(np.float32), dtype=np.float32,
                    mirror=hand[pid:pid + 1])[0]
        for row in rows:
            de, dd, _ = rc.float32_disagreement(p, t, row)
            edge, depth = max(edge, de), max(depth, dd)
            r = rc.rasterise(p, t, row, delta=rc.DELTA_PX, eps=rc.EPS_MM)
            shares.append((r["excluded"] & (r["tri"] >= 0)).sum() / r["covered"])
            covered.append(r["covered"])
    return dict(edge=edge, depth=depth, shares=np.array(shares), covered=np.array(covered))


def test_yardstick_excludes_little_and_the_constants_hold(sampled):
    s = sampled
    print(f"{len(s['shares'])} crops, {s['covered'].min()} .. {s['covered'].max()} covered pixels; float32 restatement vs float64: "
          f"edge distance {s['edge']:.3e} px (DELTA_PX {rc.DELTA_PX:.1e}), depth {s['depth']:.3e} mm (EPS_MM {rc.EPS_MM:.1e}); "
          f"excluded share of the covered pixels: max {s['shares'].max():.5f}, mean {s['shares'].mean():.5f}")
    assert len(s["shares"]) >= 100 and s["covered"].min() > 500
    assert 0 < 4 * s["edge"] <= rc.DELTA_PX and 0 < 4 * s["depth"] <= rc.EPS_MM        # the constants cover this sample
    assert rc.DELTA_PX <= 1e-3 and rc.EPS_MM <= 0.05                                     # and stay far below a pixel / a millimetre
    assert s["shares"].max() <= rc.MAX_EXCLUDED_SHARE


def test_project_landmarks_host_path_equals_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "projection_rec00.npz"))
    worst = worst_z = 0.0
    for i in range(g["landmarks"].shape[0]):
        k = int(g["case_frame"][i])
        cams = []
        for ci in range(4):
            js = dict(zip(pipeline._CAM_FIELDS, g["cams"][ci]))
            js["DistortionModel"] = "FishEye62"
            js["ImageSizeX"], js["ImageSizeY"] = int(js["ImageSizeX"]), int(js["ImageSizeY"])
            cams.append(geometry.read_camera_from_json(js).copy(camera_to_world_xf=g["c2w"][k, ci]))
        win = tracker.project_landmarks_host(cams, g["landmarks"][i])
        assert win.shape == (4, 21, 2)
        worst = max(worst, float(np.abs(win - g["window"][i]).max()))
        z = np.stack([c.world_to_eye(g["landmarks"][i].astype(np.float64))[:, 2] for c in cams])
        worst_z = max(worst_z, float(np.abs(z - g["eye_z"][i]).max()))
    print(f"host projection vs the reference: {worst:.3e} px, z {worst_z:.3e} mm over {g['landmarks'].shape[0]} cases")
    assert worst <= 1e-12 and worst_z <= 1e-12

    class Other(geometry.CameraModel):           # a model the kernel does not serve goes through its own methods
        @staticmethod
        def project(v):
            return v[..., :2] / v[..., 2, None]
    cam = Other(640, 480, (300.0, 300.0), (320.0, 240.0), geometry.NoDistortion(), np.eye(4))
    pts = np.float32([[10, 20, 500], [0, 0, 100]])
    np.testing.assert_allclose(tracker.project_landmarks([cam], pts)[0], [[326.0, 252.0], [320.0, 240.0]], atol=1e-12)
