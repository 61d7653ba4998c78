"""CPU checks that keep the resampler's edge-case table (warp_cases.py) honest, so that test_gpu_warp_edges.py cannot pass
vacuously: the float64 restatement of csrc/warp.hip's map is the oracle's map, MAP_SLACK comes from the restatement's own
float64-to-long-double spread, no in-front / behind decision hangs on rounding, every pixel class the kernel distinguishes is
populated, and the two facts about OpenCV's 8-bit arithmetic the kernel relies on hold in the oracle.

Figures of this file's checks (x86-64): 0 map mismatches of 6 580 224 entries; spread 7.96e-12, MAP_SLACK 6.4e-11; smallest
|ez| / |e| 3.8e-7; class counts in warp_cases.py's docstring."""
import numpy as np
import pytest

from oracle import ref_camera

import warp_cases as wc


@pytest.fixture(scope="module")
def table():
    """Per (size): oracle maps, float64 / long-double restatements, behind masks, |ez| / |e|, classes."""
    out = []
    for size, cams, cases in wc.tables():
        want = wc.oracle_maps(cams, cases)
        m64, behind, cosz = wc.restated_maps(cams, cases)
        mld, behind_ld, _ = wc.restated_maps(cams, cases, np.longdouble)
        out.append({"size": size, "cases": cases, "want": want, "m64": m64, "mld": mld, "behind": behind, "behind_ld": behind_ld,
                    "cosz": cosz, "classes": wc.classify(want, behind, size)})
    return out


def test_case_table_shape():
    main = wc.main_cases()
    assert len(main) == 197 and sum(c.exact for c in main) == 3 and len(wc.base_crops()) == 8
    assert len(wc.source_cameras()) == wc.N_SRC and sorted({c.src for c in main}) == sorted({s for _, s in wc.base_crops()} | {wc.AXIS_CAM, wc.FAR_CAM})
    assert len(wc.small_cases()) == 40 and len(wc.ordinary_cases()) == 8 and len(wc.behind_cases()) == 8
    mirrored = [np.linalg.det(np.asarray(c["T"])[:3, :3]) < 0 for c, _ in wc.base_crops()]
    assert any(mirrored) and not all(mirrored)                       # right hands: x-mirrored crop cameras
    for size in wc.SMALL_SIZES:
        for content in wc.CONTENTS:
            img = wc.source_images(size, content)
            assert img.shape == (wc.N_SRC,) + size and img.dtype == np.uint8
    assert wc.source_images((2, 3), "checker")[0].tolist() == [[0, 255, 0], [255, 0, 255]]
    assert wc.source_images((17, 33), "corners")[0].sum() == 4 * 255 and wc.source_images((1, 1), "corners")[0, 0, 0] == 255


def test_float64_restatement_is_the_oracle_map(table):
    """The restatement written in the kernel's order of operations, cast to float32, is ref_camera.warp_map entry for entry,
    and puts the same pixels behind the camera."""
    differ = total = 0
    for t in table:
        differ += int((t["m64"].astype(np.float32) != t["want"]).sum())
        total += t["want"].size
        assert np.array_equal(t["behind"], (t["want"] == -1).all(-1)) and np.array_equal(t["behind"], t["behind_ld"]), t["size"]
    print(f"restatement vs oracle: {differ} mismatches of {total}")
    assert differ == 0


def test_map_slack_covers_the_reference_spread(table):
    """MAP_SLACK >= 8 x the largest float64-to-long-double distance of the restated map over the pixels in front; outside the
    exact cases no pixel has |ez| / |e| < 1e-9, so no behind decision depends on rounding."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: the spread cannot be measured")
    spread, margin = 0.0, np.inf
    for t in table:
        front = ~t["behind"]
        d = np.abs(t["m64"].astype(np.longdouble) - t["mld"]) / np.maximum(1, np.abs(t["mld"]))
        spread = max(spread, float(d[front].max()))
        margin = min(margin, float(t["cosz"][[not c.exact for c in t["cases"]]].min()))
    print(f"float64 vs long double: {spread:.3e}; MAP_SLACK {wc.MAP_SLACK:.3e}; smallest |ez|/|e| {margin:.3e}")
    assert wc.MAP_SLACK == 8 * wc.MAP_SPREAD and wc.MAP_SLACK >= 8 * spread
    assert wc.MAP_SLACK < 2.0 ** -24 / 64            # far below half a float32 ulp of a coordinate >= 1: the slack decides ties only
    assert margin >= wc.EZ_MARGIN


def test_exact_cases_are_exact(table):
    """The hand-written rotations: on the axis the map is the source's principal point, looking backwards gives (-1, -1), and the
    exact quarter turn has ez == 0 at the centre (not behind) with theta == pi / 2."""
    main = table[0]
    idx = {c.name: i for i, c in enumerate(main["cases"]) if c.exact}
    cam = wc.source_cameras()[wc.AXIS_CAM]
    centre = np.array([cam["c"][0], cam["c"][1]], np.float64)
    assert np.array_equal(main["m64"][idx["identity"], 48, 48], centre)
    assert np.array_equal(main["want"][idx["identity"], 48, 48], centre.astype(np.float32))
    assert main["behind"][idx["backwards"]].all() and (main["want"][idx["backwards"]] == -1).all()
    q = idx["quarter_turn"]
    assert main["cosz"][q, :, 48].max() == 0 and not main["behind"][q, :, 48].any()
    assert main["behind"][q, :, 49:].all() and not main["behind"][q, :, :48].any()
    # theta == pi / 2 on the x axis: the closed form of the projection, y exactly on the principal row
    k1, k2, k3, k4, p1, p2, k5, k6 = cam["k"]
    u = np.arctan2(1.0, 0.0)
    r2 = u * u
    r4, r6 = r2 * r2, r2 * r2 * r2
    x = u * (1 + k1 * r2 + k2 * r4 + k3 * r6 + k4 * (r4 * r4) + k5 * (r4 * r6) + k6 * (r6 * r6))
    want = np.array([(x + (2 * p2 * 0.0 + p1 * (x * x + 2 * (x * x)))) * cam["f"][0] + cam["c"][0],
                     (0.0 + (2 * p1 * 0.0 + p2 * (x * x + 2 * 0.0))) * cam["f"][1] + cam["c"][1]])
    assert np.array_equal(main["m64"][q, 48, 48], want)


def test_every_pixel_class_is_covered(table):
    """At least 1000 pixels of every class over the whole table, a crop fully behind and one fully inside, and straddling pixels
    on all four sides at every small size."""
    total = {k: 0 for k in wc.CLASSES}
    fully = {"behind": 0, "inside": 0}
    for t in table:
        counts = {k: int(v.sum()) for k, v in t["classes"].items()}
        print(t["size"], counts)
        for k in wc.CLASSES:
            total[k] += counts[k]
        for k in fully:
            fully[k] += int(t["classes"][k].all((1, 2)).sum())
        # every pixel is in a class (one at a corner of the image in two)
        assert (sum(v.astype(int) for v in t["classes"].values()) >= 1).all()
        if t["size"] != wc.BIG:
            for side in ("left", "right", "top", "bottom"):
                assert counts[side] > 0, (t["size"], side)
    print("total", total, "crops fully", fully)
    for k in wc.CLASSES:
        assert total[k] >= 1000, (k, total[k])
    assert fully["behind"] >= 1 and fully["inside"] >= 1
    main = table[0]
    # what the fused-path test builds its all-1.0 and all-zero crops from
    assert int(main["classes"]["inside"][wc.ordinary_cases()].all((1, 2)).sum()) >= 4 and main["behind"][wc.behind_cases()].all()
    # the integer sampler meets negative 1/32-pixel coordinates with a fraction, and both samplers every range they clamp to:
    # beyond +-32768 px, beyond +-1e6 px (float sampler) and beyond +-1e9 / 32 px (integer sampler)
    front = np.broadcast_to(~main["behind"][..., None], main["want"].shape)
    sx = np.rint(main["want"].astype(np.float64) * 32)
    a = np.abs(main["want"][front].astype(np.float64))
    ranges = {"negative fraction": int(((sx < 0) & (sx % 32 != 0) & front).sum()), "32768 .. 1e6": int(((a > 32768) & (a < 1e6)).sum()),
              "1e6 .. 1e9/32": int(((a > 1e6) & (a < 1e9 / 32)).sum()), "> 1e9/32": int((a > 1e9 / 32).sum())}
    print(ranges)
    assert min(ranges.values()) >= 1000, ranges


def test_closed_form_weights_are_opencvs_table():
    """csrc/warp.hip computes the four 15-bit weights as (32 - ay)(32 - ax) * 32 etc. instead of reading OpenCV's table: the two
    agree at all 32 x 32 fractions (every product is an exact multiple of 32, so nothing is rounded and no residual is moved)."""
    tab = ref_camera.cv2_bilinear_tab()
    ay, ax = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    closed = np.stack(((32 - ay) * (32 - ax) * 32, (32 - ay) * ax * 32, ay * (32 - ax) * 32, ay * ax * 32), -1)
    assert tab.shape == closed.shape == (32, 32, 4) and np.array_equal(tab, closed)
    assert tab[0, 0].tolist() == [32768, 0, 0, 0] and (tab.sum(-1) == 32768).all()


@pytest.mark.parametrize("mode", ["cv2", "float"])
def test_behind_marker_samples_zero(mode):
    """(-1, -1), what a pixel behind the camera is mapped to, samples the constant border only: 0, even when source pixel (0, 0)
    is 255 (its weight at fraction 0 is 0)."""
    src = np.zeros((5, 7), np.uint8)
    src[0, 0] = 255
    m = np.full((2, 3, 2), -1, np.float32)
    out = ref_camera.remap_bilinear(src, m, mode)
    assert out.shape == (2, 3) and (out == 0).all()
    m[0, 0] = (-0.5, -0.5)                                     # the check above is not vacuous: half a pixel in, a quarter of 255
    assert ref_camera.remap_bilinear(src, m, mode)[0, 0] == (64 if mode == "cv2" else 63.75)
