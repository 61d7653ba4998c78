"""GPU tests of the fisheye -> pinhole crop resampler (csrc/warp.hip: ut_warp_map, ut_warp_crops, the u8 / fp32 front of
ut_warp_backbone) at the edges the parity tests' fully visible hands never reach: the constant-0 border on all four sides in both
samplers, negative and far-out coordinates up to every clamp, pixels behind the source camera, rays on the source axis and at 90
degrees to it, sources from 1 x 1 to 480 x 636, calls cut into several launches, and all-zero / all-255 crops entering the stem.

The cases, the float64 restatement of the map and MAP_SLACK come from warp_cases.py; test_warp_host.py shows on the CPU that the
restatement is the oracle's map and that every pixel class is populated.  Every comparison is against oracle.ref_camera or that
restatement.  Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from absolutetrack_amd import _native, geometry, synth
from oracle import ref_camera

import warp_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"cv2": _native.UT_REMAP_CV2_FIXED, "float": _native.UT_REMAP_FLOAT}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Table:
    """One table of warp_cases.tables() packed for the kernels, the source camera rows in scrambled order, with the oracle's
    float32 maps, the float64 restatement and the behind masks."""

    def __init__(self, size, cams, cases, seed):
        self.size, self.cases, self.n = size, cases, len(cases)
        self.perm = np.random.default_rng(seed).permutation(len(cams))            # row j of the table is camera perm[j]
        self.src = np.array([c.src for c in cases])
        self.cam_rows = np.stack([geometry.pack_source_camera(c["f"], c["c"], c["k"], c["T"]) for c in cams])
        self.crop_rows = np.stack([geometry.pack_crop_camera(c.crop["f"], c.crop["c"], c.crop["T"]) for c in cases])
        self.want32 = wc.oracle_maps(cams, cases)
        self.want64, self.behind, _ = wc.restated_maps(cams, cases)
        self.classes = wc.classify(self.want32, self.behind, size)

    def args(self, rows=None, perm=None):
        """(cam table, crop rows, src_index) on the device for the cases `rows` (all by default) under `perm`."""
        perm = self.perm if perm is None else perm
        rows = np.arange(self.n) if rows is None else np.asarray(rows)
        return _dev(self.cam_rows[perm]), _dev(self.crop_rows[rows]), _dev(np.argsort(perm)[self.src[rows]].astype(np.int32))

    def images(self, content, perm=None):
        """Source images in the camera table's order (device), and in the cameras' own order (numpy)."""
        img = wc.source_images(self.size, content, n=len(self.perm))
        return _dev(img[self.perm if perm is None else perm]), img


@pytest.fixture(scope="module")
def tables():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return [Table(size, cams, cases, seed=i) for i, (size, cams, cases) in enumerate(wc.tables())]


@pytest.fixture(scope="module")
def engine(tables):
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    yield eng
    eng.close()


def _gpu_map(t, rows=None, perm=None):
    cam, crop, idx = t.args(rows, perm)
    return _native.warp_map(cam, crop, idx, cam.shape[0])


def test_map_against_float64(tables):
    """ut_warp_map on every case (197 crops on the 10 full-size source cameras in one call, 40 per small size) against the float64
    restatement: every entry in front is one of the two float32 values that bracket the float64 one, within half a float32 ulp +
    MAP_SLACK x max(1, |value|) of it; exactly the oracle's behind pixels are (-1, -1); the exact cases give their closed forms.
    MI355X: not recorded yet; the test prints, per table, the entries that are not float32(want64) and the largest error / bound."""
    differ = total = 0
    worst, main_got = 0.0, None
    for t in tables:
        got = _gpu_map(t).cpu().numpy()
        main_got = got if t is tables[0] else main_got
        assert got.shape == t.want64.shape == (t.n, 96, 96, 2)
        behind = np.broadcast_to(t.behind[..., None], got.shape)
        assert np.array_equal((got == -1).all(-1), t.behind), t.size               # those and no others
        assert np.array_equal(t.behind, (t.want32 == -1).all(-1))
        g, w = got[~behind], t.want64[~behind]
        lo, hi = wc.bracket32(w)
        err = np.abs(g.astype(np.float64) - w)
        bound = wc.ulp32(w) / 2 + wc.MAP_SLACK * np.maximum(1, np.abs(w))
        n_off = int((g != w.astype(np.float32)).sum())
        differ, total, worst = differ + n_off, total + g.size, max(worst, float((err / bound).max()))
        print(f"{t.size}: {n_off} of {g.size} entries in front differ from float32(want64); largest error / bound "
              f"{float((err / bound).max()):.4f}; {int((got != t.want32).sum())} differ from the oracle's map")
        assert ((g == lo) | (g == hi)).all(), (t.size, int((~((g == lo) | (g == hi))).sum()))
        assert (err <= bound).all(), (t.size, int((err > bound).sum()), float((err / bound).max()))
    print(f"all tables: {differ} of {total} differ from float32(want64); largest error / bound {worst:.4f}")
    main, got = tables[0], main_got
    idx = {c.name: i for i, c in enumerate(main.cases) if c.exact}
    cam = wc.source_cameras()[wc.AXIS_CAM]
    assert got[idx["identity"], 48, 48].tolist() == [np.float32(cam["c"][0]), np.float32(cam["c"][1])]        # r == 0
    assert (got[idx["backwards"]] == -1).all()
    q = idx["quarter_turn"]                                                        # ez == 0 is in front, theta == pi / 2
    assert np.array_equal(got[q, 48, 48], main.want32[q, 48, 48]) and (got[q, :, :49] != -1).all() and (got[q, :, 49:] == -1).all()


def _oracle_sampler(t, src, maps, mode):
    """ref_camera.remap_bilinear of every case of table t at `maps`, / 255 in float32 as the kernel does: one call per source
    image, over all the crops that read it."""
    out = np.empty(maps.shape[:3], np.float32)
    for s in np.unique(t.src):
        rows = np.flatnonzero(t.src == s)
        v = ref_camera.remap_bilinear(src[s], maps[rows].reshape(-1, 96, 2), mode)
        out[rows] = (v.astype(np.float32) / np.float32(255)).reshape(len(rows), 96, 96)
    return out


def _check_sampling(engine, t, mode, bound):
    """ut_warp_crops + ut_warp_map on table t (480 x 636: noise sources; a small size: every content), against the oracle's
    sampler on the GPU's map (within `bound`) and on the oracle's own map (a pixel may differ only where the maps do)."""
    cam, crop, idx = t.args()
    gmap = _native.warp_map(cam, crop, idx, cam.shape[0]).cpu().numpy()
    map_differs = (gmap != t.want32).any(-1)
    pixels = unequal = off_map = 0
    worst = 0.0
    for content in (("noise",) if t.size == wc.BIG else wc.CONTENTS):
        src_dev, src = t.images(content)
        got = engine.warp_crops(src_dev, cam, crop, idx, MODES[mode]).cpu().numpy()
        want = _oracle_sampler(t, src, gmap, mode)
        e2e = _oracle_sampler(t, src, t.want32, mode) if map_differs.any() else want
        assert got.shape == want.shape == (t.n, 96, 96)
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst, unequal, pixels = max(worst, err), unequal + int((got != want).sum()), pixels + got.size
        assert err <= bound, (t.size, content, err, int((got != want).sum()))
        assert not ((got != e2e) & ~map_differs).any(), (t.size, content)
        off_map += int((got != e2e).sum())
        assert got[t.behind].max(initial=0) == 0
    print(f"{mode} sampler, {t.size}: largest error {worst:.3e} (bound {bound:.3e}); {unequal} of {pixels} pixels not bit-equal given "
          f"the map; {off_map} differ end to end, all among the {int(map_differs.sum())} pixels whose map entries differ")


TABLE_IDS = [f"{h}x{w}" for h, w in (wc.BIG,) + wc.SMALL_SIZES]


@pytest.mark.parametrize("ti", range(len(TABLE_IDS)), ids=TABLE_IDS)
def test_sampling_given_the_map_cv2(engine, tables, ti):
    """ut_warp_crops in the OpenCV-style mode against the oracle's integer sampler fed the map ut_warp_map returned in the same
    test: 0 differing pixels over all 197 crops on 480 x 636 noise and over all 40 crops of every (small size, content) pair.
    Against the oracle end to end a pixel may differ only where the maps differ.
    MI355X: not recorded yet; the test prints the pixel counts per table."""
    _check_sampling(engine, tables[ti], "cv2", 0.0)


@pytest.mark.parametrize("ti", range(len(TABLE_IDS)), ids=TABLE_IDS)
def test_sampling_given_the_map_float(engine, tables, ti):
    """The same in float mode.  Each tap product (u8 x float32 weight) is exact in float64 and the four-term sum runs in the same
    order on both sides, so the bound is one float32 ulp of the result, 2^-24 on [0, 1]; bit equality is expected.
    MI355X: not recorded yet; the test prints the largest error and the count of pixels that are not bit-equal per table."""
    _check_sampling(engine, tables[ti], "float", 2.0 ** -24)


@pytest.mark.parametrize("mode", ["cv2", "float"])
def test_crops_behind_the_camera_are_zero(engine, tables, mode):
    """Crops fully behind the source camera sample (-1, -1) everywhere: all zeros in both modes although source pixel (0, 0) is
    255 ("all255" and "corners" sources).  Crops fully inside the all-255 source are all 1.0: exactly in the integer mode (the
    weights sum to 32768); within 8 x 2^-24 in float mode (four weights, each a rounded product of two rounded factors: <= 3 x
    2^-24 of the sum together; the conversion to float32 and the division by 255: 2^-24 each)."""
    t = tables[0]
    inside = [i for i in wc.ordinary_cases() if t.classes["inside"][i].all()]
    rows = wc.behind_cases() + inside
    assert len(inside) >= 4 and t.behind[wc.behind_cases()].all()
    cam, crop, idx = t.args(rows)
    for content in ("all255", "corners"):
        src_dev, src = t.images(content)
        assert (src[:, 0, 0] == 255).all()
        got = engine.warp_crops(src_dev, cam, crop, idx, MODES[mode])
        assert int(torch.count_nonzero(got[:8])) == 0, content
        if content == "all255":
            assert float((got[8:] - 1.0).abs().max()) <= (0.0 if mode == "cv2" else 8 * 2.0 ** -24)


def _fused_batch(t):
    """Source images / camera table / crops / src_index of the fused-path test: 10 noise images then 10 all-255 images under the
    same 10 cameras; the 8 ordinary crops on noise, the 8 fully-behind crops on the all-255 images (all-zero crops), the fully
    inside ordinary crops on the all-255 images (all-1.0 crops - to rounding in float mode: grey level 255 in the u8 stem)."""
    n_src = len(t.perm)
    inside = [i for i in wc.ordinary_cases() if t.classes["inside"][i].all()]
    rows = wc.ordinary_cases() + wc.behind_cases() + inside
    white = np.array([False] * 8 + [True] * (8 + len(inside)))
    src = np.concatenate([wc.source_images(t.size, "noise", n=n_src), wc.source_images(t.size, "all255", n=n_src)])
    idx = (t.src[rows] + n_src * white).astype(np.int32)
    return _dev(src), _dev(np.concatenate([t.cam_rows, t.cam_rows])), _dev(t.crop_rows[rows]), _dev(idx), len(inside)


@pytest.mark.parametrize("mode", ["cv2", "float"])
@pytest.mark.parametrize("conv", ["fp32", "split_f16_always"])
def test_fused_path_on_edge_crops(tables, conv, mode):
    """ut_warp_backbone == ut_backbone(ut_warp_crops) bit for bit on a batch that mixes ordinary crops with all-zero crops (fully
    behind the camera) and all-1.0 crops (the all-255 source), and on a batch of all-zero crops alone: finite features, and
    poll_status() raises no range check.  Both convolution arithmetics, both remap modes.
    MI355X: not recorded yet; the test prints the largest feature magnitude of both batches."""
    t = tables[0]
    eng = _native.HipEngine(synth.synthetic_state_dict(0), DEV)
    try:
        eng.set_conv_arithmetic(conv)
        src, cam, crop, idx, n_inside = _fused_batch(t)
        assert n_inside >= 4
        crops = eng.warp_crops(src, cam, crop, idx, MODES[mode])
        assert int(torch.count_nonzero(crops[8:16])) == 0
        assert float((crops[16:] - 1.0).abs().max()) <= (0.0 if mode == "cv2" else 8 * 2.0 ** -24)
        assert 0.3 < float(crops[:8].mean()) < 0.7 and float(crops[:8].std()) > 0.05          # the ordinary ones: noise
        want = eng.backbone(crops)
        got = eng.warp_backbone(src, cam, crop, idx, MODES[mode])
        assert got.shape == want.shape == (16 + n_inside, 72, 6, 6) and torch.equal(got, want)
        assert bool(torch.isfinite(got).all())
        # every crop all-zero
        zero = eng.warp_backbone(src, cam, crop[8:16], idx[8:16], MODES[mode])
        eng.poll_status()
        assert bool(torch.isfinite(zero).all())
        assert torch.equal(zero, eng.backbone(torch.zeros(8, 96, 96, device=DEV)))
        eng.poll_status()
        print(f"{conv} / {mode}: largest |feature| mixed batch {float(got.abs().max()):.4f}, all-zero batch {float(zero.abs().max()):.4f}")
    finally:
        eng.close()


def test_batch_independence(engine, tables):
    """A crop's map and image do not depend on its batch: the 197-crop call equals the same crops one per call, and the same crops
    with the camera table, the images and src_index under another permutation, bit for bit (map, and both image modes)."""
    t = tables[0]
    cam, crop, idx = t.args()
    src, _ = t.images("noise")
    whole = [_native.warp_map(cam, crop, idx, cam.shape[0])] + [engine.warp_crops(src, cam, crop, idx, m) for m in MODES.values()]
    for i in range(t.n):
        c, k = crop[i:i + 1], idx[i:i + 1]
        one = [_native.warp_map(cam, c, k, cam.shape[0])] + [engine.warp_crops(src, cam, c, k, m) for m in MODES.values()]
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, whole)), t.cases[i].name
    perm = np.roll(t.perm[::-1], 3)
    assert not np.array_equal(perm, t.perm)
    cam2, crop2, idx2 = t.args(perm=perm)
    src2, _ = t.images("noise", perm=perm)
    again = [_native.warp_map(cam2, crop2, idx2, cam2.shape[0])] + [engine.warp_crops(src2, cam2, crop2, idx2, m) for m in MODES.values()]
    assert all(torch.equal(a, b) for a, b in zip(again, whole))
    # and in another crop order
    order = np.random.default_rng(5).permutation(t.n)
    o = _dev(order)
    shuffled = [_native.warp_map(cam, crop[o], idx[o], cam.shape[0])] + [engine.warp_crops(src, cam, crop[o], idx[o], m) for m in MODES.values()]
    assert all(torch.equal(a, b[o]) for a, b in zip(shuffled, whole))


def test_more_than_one_launch_per_call(engine, tables):
    """32776 crops (32768 + 8: launch_warp / launch_warp_map cut a call at 32768 crops and offset crop, src_index and out for the
    second launch), cycling 8 distinct (crop camera, source) pairs: viewed as [4097, 8, ...] every row equals row 0 (compared on
    the device) and row 0 equals an 8-crop call.  1.2 GB of images, then 2.4 GB of map; 8 crops reach the host."""
    t = tables[0]
    names = ("b0.f1.0.r0", "b1.f0.5.r0", "b2.f0.25.r30", "b3.f0.1.r60", "b4.f1.0.r90", "b5.f0.5.r120", "b6.f1.0.r0", "identity")
    rows = [[c.name for c in t.cases].index(n) for n in names]
    assert len({t.src[r] for r in rows}) >= 4
    cam, crop8, idx8 = t.args(rows)
    src, _ = t.images("noise")
    n, reps = 32776, 4097
    crop, idx = crop8.repeat(reps, 1), idx8.repeat(reps)
    assert crop.shape == (n, 24) and idx.shape == (n,)

    def rows_equal(out, want8):
        v = out.view(reps, -1)
        return torch.equal(v[0], want8.reshape(-1)) and bool((v == v[:1]).all())

    want8 = engine.warp_crops(src, cam, crop8, idx8, MODES["cv2"])
    out = engine.warp_crops(src, cam, crop, idx, MODES["cv2"])
    assert out.shape == (n, 96, 96) and rows_equal(out, want8)
    first = want8.cpu().numpy()
    assert 0 < np.count_nonzero(first) < first.size
    del out
    torch.cuda.empty_cache()
    want8 = _native.warp_map(cam, crop8, idx8, cam.shape[0])
    out = _native.warp_map(cam, crop, idx, cam.shape[0])
    assert out.shape == (n, 96, 96, 2) and rows_equal(out, want8)
    del out
    torch.cuda.empty_cache()
