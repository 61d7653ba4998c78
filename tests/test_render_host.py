"""CPU tests of the rendered hand: the C declarations, the host refusals of ut_project_points / ut_render_mesh, the float64
yardstick rasteriser of tests/render_cases.py against an image worked out by hand, the yardstick's own excluded share and the
constants DELTA_PX / EPS_MM against a re-measurement, the host path of project_landmarks against the reference's numbers, and
the exact lattice cases of tests/render_cases.py (float64, float32 and int64 draw one picture; every wrong rule is caught)."""
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


# ----------------------------------------------------------------------------- exact geometry: the lattice cases
# The cases tests/test_gpu_render_rules.py draws on the GPU, checked here first: that they are exact (float64, float32 and
# integer arithmetic draw one picture, no pixel left out), that they say what they claim, and that they tell the renderer's
# rules from the mistakes a renderer could make.
CAUGHT_BY = {"inclusive": ("sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "ties", "hand_case", "sloped"),
             "exclusive": ("sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "ties", "hand_case", "near"),
             "bottom_right": ("sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "ties", "hand_case", "sloped"),
             "top_left_before_exchange": ("sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "mirrored", "mirrored_hand"),
             "higher_index": ("ties",),
             "cull_negative": ("sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "mirrored_hand", "near")}


@pytest.fixture(scope="module")
def lattice():
    """Every case, and per (pose, crop) of it: the float64 yardstick, the float32 restatement, their disagreement (not for
    `hostile`, whose distances are not numbers) and the integer restatement (for `hostile`: the bare sheet only)."""
    cases = rc.lattice_cases()
    out = {}
    for name, c in cases.items():
        per = {}
        for p, k in rc.case_crops(c):
            v, t, row = c["vertices"][p], c["triangles"], c["crop_rows"][k]
            with np.errstate(all="ignore"):
                r64, r32 = rc.rasterise(v, t, row), rc.rasterise(v, t, row, np.float32)
                dis = rc.float32_disagreement(v, t, row)[:2] if name != "hostile" else None
            whole = name != "hostile" or p == 0
            per[p, k] = dict(r64=r64, r32=r32, dis=dis, int=rc.rasterise_int(v, t, row) if whole else None)
        out[name] = (c, per)
    return out


def test_lattice_cases_are_named_and_small(lattice):
    assert list(lattice) == ["hand_case", "sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "degenerate", "ties",
                             "mirrored", "mirrored_hand", "sloped", "near", "hostile", "batch"]
    for name, (c, per) in lattice.items():
        n_p, n_v = c["vertices"].shape[:2]
        assert c["vertices"].dtype == np.float32 and c["triangles"].dtype == np.int32 and c["sample_range"].shape == (n_p, 2)
        assert 0 <= c["triangles"].min() and c["triangles"].max() < n_v <= rc.RENDER_MAX_VERTICES, name      # every index in range
        assert len(per) == len(c["crop_rows"]) <= 4 and np.isfinite(c["vertices"][0]).all(), name            # pose 0 makes the Mesh
        again = rc.lattice_cases()[name]
        assert all(np.array_equal(c[k], again[k], equal_nan=c[k].dtype.kind == "f") for k in ("vertices", "triangles", "crop_rows")), name
    d = lattice["sheet_dense"][0]
    assert d["vertices"].shape[1] == rc.RENDER_MAX_VERTICES and len(d["triangles"]) == 4418 > 17 * 256
    assert lattice["batch"][0]["sample_range"].tolist() == [[0, 2], [2, 2], [2, 3]]


def test_lattice_condition_holds(lattice):
    """Asserted from the vertices: every projected coordinate a multiple of a quarter pixel, every difference inside a drawn
    triangle below 512 px (2048 px on the integer lattice) - so each edge function fits fp32's 24 bits."""
    for name, (c, _) in lattice.items():
        with np.errstate(invalid="ignore"):                     # hostile: NaN and inf go through the projection
            quarter, integer = rc.lattice_extents(c)
        print(f"{name}: largest coordinate difference inside a triangle {quarter} px (quarter lattice), {integer} px (integer lattice)")
        assert quarter < rc.LATTICE_LIMIT_QUARTER and integer < rc.LATTICE_LIMIT_INTEGER, name
        tris = c["triangles"].astype(np.int64)
        for (p, k), r in per_crop(lattice, name):
            drawn = np.unique(r["r64"]["tri"][r["r64"]["tri"] >= 0])
            ok = c["on_lattice"][p][tris[drawn]].all(1)
            if name == "hostile":                               # the float64 rules also draw what overflows float32
                ok |= np.isin(drawn, c["overflow_triangles"])
            assert ok.all(), (name, p, k, drawn[~ok])           # nothing is drawn from a vertex that is off the lattice


def per_crop(lattice, name):
    return lattice[name][1].items()


def test_three_arithmetics_draw_one_picture(lattice):
    """float64 = float32 = int64, every pixel of every case; where the integer restatement cannot order depths (a sloped
    triangle) it must still cover the same pixels."""
    for name, (c, per) in lattice.items():
        for (p, k), r in per.items():
            r64, r32 = r["r64"], r["r32"]
            if name == "hostile" and p >= 2:
                # nothing hides the triangles whose float32 area overflows: float64 draws them, float32 must not, and the
                # two pictures differ nowhere else
                over = np.isin(r64["tri"], c["overflow_triangles"])
                assert over.any() and np.array_equal(r64["tri"][~over], r32["tri"][~over]) and not np.isin(r32["tri"], c["overflow_triangles"]).any()
                continue
            assert np.array_equal(r64["tri"], r32["tri"]), (name, p, k)
            if r["int"] is None:
                continue
            if r["int"]["tri"] is not None:
                assert np.array_equal(r["int"]["tri"], r64["tri"]), (name, p, k)
            else:
                assert name in ("hand_case", "mirrored_hand", "sloped")
                assert np.array_equal(r["int"]["count"] > 0, r64["tri"] >= 0), (name, p, k)
            if c.get("single_owner"):
                assert (r["int"]["count"] == 1).all(), (name, p, k)


def test_lattice_cases_show_what_they_claim(lattice):
    for name, (c, per) in lattice.items():
        for (p, k), r in per.items():
            y = r["r64"]
            if c.get("single_owner"):
                assert y["covered"] == 9216 and np.isinf(y["depth2"]).all(), (name, p, k)          # each pixel once
            if name != "hostile":
                n_edge = rc.on_edge_count(c["vertices"][p], c["triangles"], c["crop_rows"][k])
                print(f"{name} pose {p} crop {k}: {y['covered']} pixels covered, {n_edge} pixel centres on an edge")
                assert n_edge > 0, (name, p, k)                                                      # the fill rule decides somewhere
    count = lambda name, key, t: int((lattice[name][1][key]["r64"]["tri"] == t).sum())
    for name, keys in (("hand_case", [(0, 0)]), ("mirrored_hand", [(0, 0), (0, 1)])):
        for key in keys:
            y = lattice[name][1][key]["r64"]
            assert y["covered"] == 62 and [count(name, key, t) for t in range(4)] == [26, 36, 0, 0]
    y = lattice["hand_case"][1][0, 0]["r64"]
    assert y["depth"][0, 0] == 128.0 and abs(y["depth"][2, 6] - 256 / 3) < 1e-12 and abs(y["depth"][4, 4] - 512 / 7) < 1e-12
    ym = lattice["mirrored_hand"][1][0, 1]["r64"]
    flipped = lattice["mirrored_hand"][1][0, 0]["r64"]["tri"][:, 20::-1]
    assert (ym["tri"][:, :21] != flipped).any()             # not the flipped picture: x = 20 is a right edge now
    # the dense sheet crosses rows 47 / 48, leaves on the left and at the top, and ends inside on the right and at the bottom
    y = lattice["sheet_dense"][1][0, 0]["r64"]["tri"]
    assert (y[47:49, :60] >= 0).all() and (y[0, :60] >= 0).all() and (y[:80, 0] >= 0).all() and (y[:, 70:] < 0).all() and (y[90:] < 0).all()
    assert lattice["sheet_dense"][0]["triangles"].max() < 2304
    # seam: a horizontal edge on row 48 belongs to the triangle below it (its top edge), one on 47 likewise, 47.5 touches no centre
    c, y = lattice["seam"][0], lattice["seam"][1][0, 0]["r64"]["tri"]
    assert (y[48, 3:20] == 0).all() and (y[47, 3:20] == 1).all() and (y[47, 25:40] == 3).all() and (y[46, 26:39] == 2).all()
    assert (y[47, 46:59] == 4).all() and (y[48, 46:59] == 5).all() and set(np.unique(y[:, 64:91])) >= {6, 7, 9}
    assert y[47, 68] == 6 and y[48, 88] == 6 and y[48, 69] == 7          # 7's vertices on the centres (68,47), (88,48) are not its own
    assert y[55, 66] == 6 and (y[56, 60:] < 0).all() and (y[40, 60:] < 0).all() and y[41, 65] == 6      # (66,56), (64,40): vertices of 6
    # borders: nothing from the triangles outside or between centres; column 95 and row 95 follow the fill rule
    c, y = lattice["borders"][0], lattice["borders"][1][0, 0]["r64"]
    lo, hi = c["n_nothing"]
    assert not np.isin(y["tri"], np.arange(lo, hi)).any() and y["covered"] == 9216 and (y["tri"][60:62, 10:31] == 19).all()
    assert y["tri"][0, 0] == 0 and (y["tri"][:10, 95] == 19).all() and y["tri"][0, 94] == 1           # x = 95 as a right edge: not covered
    assert (y["tri"][41:50, 95] == 4).all() and (y["tri"][41:50, 0] == 3).all() and (y["tri"][95, 20:31] == 19).all()
    assert (y["tri"][95, 61:69] == 7).all() and (y["tri"][0, 61:69] == 8).all() and y["tri"][95, 0] == 19 and y["tri"][94, 0] == 9
    assert (y["tri"][21:29, 95] == 2).all() and (y["tri"][87:95, 40] == 6).all()      # x = 96 lies outside: column 95 is inside
    # degenerate: the sheet's picture, bit for bit
    a, b = lattice["degenerate"][1][0, 0]["r64"], lattice["sheet_integer"][1][0, 0]["r64"]
    assert all(np.array_equal(a[k], b[k]) for k in ("tri", "depth", "shade", "depth2"))
    # ties
    y = lattice["ties"][1][0, 0]["r64"]
    assert count("ties", (0, 0), 5) == 36 * 37 // 2 and count("ties", (0, 0), 4000) == 0 and (y["depth2"][y["tri"] == 5] == 128).all()
    assert y["tri"][12, 62] == 6 and y["tri"][8, 62] == 7 and y["tri"][12, 55] == 7 and y["tri"][40, 62] == 6 and y["depth2"][12, 62] == 128
    assert y["tri"][60, 12] == 3000 and y["depth"][60, 12] == 64 and y["tri"][52, 12] == 10 and y["depth2"][60, 12] == 128
    assert count("ties", (0, 0), 20) > 0 and count("ties", (0, 0), 2999) > 0
    # near
    y = lattice["near"][1][0, 0]["r64"]
    assert set(np.unique(y["tri"])) == {3, 4, 5} and count("near", (0, 0), 3) == 96 * 97 // 2 and y["tri"][0, 95] == 3 and y["tri"][1, 95] == 4
    assert float(rc.NEAR_F32) < rc.NEAR < float(rc.NEAR_KEPT) and (np.abs(y["depth"][y["tri"] == 3] - float(rc.NEAR_KEPT)) < 1e-19).all()
    # hostile: in front of or without the unusual triangles the sheet's picture; the ordinary triangle among them is drawn
    c, per = lattice["hostile"]
    bare = per[0, 0]["r64"]
    assert all(np.array_equal(bare[k], lattice["sheet_integer"][1][0, 0]["r64"][k]) for k in ("tri", "depth", "shade"))
    for key in ((1, 1),):
        assert all(np.array_equal(per[key][dt][k], bare[k]) for dt in ("r64", "r32") for k in ("tri", "depth", "shade"))
    for key in ((2, 2), (3, 3)):
        y = per[key]["r32"]
        assert (y["tri"] == c["plain_triangle"]).sum() == 32 * 33 // 2 and not np.isin(y["tri"], np.arange(c["n_sheet"], c["plain_triangle"])).any()
    assert (per[3, 3]["r32"]["tri"] >= 0).sum() == 32 * 33 // 2


def test_exact_depth_cases(lattice):
    """Which cases the GPU test may hold to float32(z) exactly, and the disagreement that bounds the others."""
    for name, (c, per) in lattice.items():
        if name == "hostile":
            continue
        for (p, k), r in per.items():
            edge, depth = r["dis"]
            hit = r["r64"]["tri"] >= 0
            print(f"{name} pose {p} crop {k}: float32 restatement vs float64: edge distance {edge:.3e} px, depth {depth:.3e} mm")
            assert edge == 0.0, (name, p, k)                                   # every edge function is exact
            if name in rc.EXACT_DEPTH_CASES:
                assert depth == 0.0 and np.array_equal(r["r32"]["depth"], r["r64"]["depth"]), (name, p, k)
                z = r["r64"]["depth"][hit]
                assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and set(np.unique(z)) <= {64.0, 128.0, 256.0}
            else:
                assert 0 < depth < 1e-5 and np.abs(r["r32"]["depth"][hit] - r["r64"]["depth"][hit]).max() <= depth, (name, p, k)
    assert set(lattice) - set(rc.EXACT_DEPTH_CASES) == {"hand_case", "mirrored_hand", "sloped", "near", "hostile"}
    # the sloped sheets: 1 / z crosses between two pixel columns (B ends on x + y = 95), and the nearest two surfaces are never close
    for key, least in (((0, 0), 0.3), ((1, 1), 0.14)):
        y = lattice["sloped"][1][key]["r64"]
        xs, ys = np.meshgrid(np.arange(96), np.arange(96))
        assert np.array_equal(y["tri"] == 1, (xs < 48) & (xs + ys < 95)) and (y["tri"] >= 0).all()
        assert (y["depth2"] - y["depth"])[np.isfinite(y["depth2"])].min() > least


def test_every_wrong_rule_changes_a_named_case(lattice):
    """The cases discriminate: each mistake in rc.RULES changes the integer restatement's picture (the owner, or where depths
    cannot be ordered the coverage count) of every case CAUGHT_BY names for it."""
    caught = {rule: [] for rule in rc.RULES[1:]}
    for name, (c, per) in lattice.items():
        for (p, k), r in per.items():
            if r["int"] is None:
                continue
            what = "tri" if r["int"]["tri"] is not None else "count"
            for rule in rc.RULES[1:]:
                wrong = rc.rasterise_int(c["vertices"][p], c["triangles"], c["crop_rows"][k], rule)
                n = int((wrong[what] != r["int"][what]).sum())
                if n and name not in caught[rule]:
                    caught[rule].append(name)
    for rule, names in caught.items():
        print(f"rule '{rule}' changes the picture of: {', '.join(names)}")
    assert set(CAUGHT_BY) == set(rc.RULES[1:])
    for rule, names in CAUGHT_BY.items():
        for name in names:
            assert name in caught[rule], f"the wrong rule '{rule}' draws the case '{name}' like the right one: the case no longer catches it"
