"""Shared by the edge tests of the fisheye -> pinhole crop resampler (test_warp_host.py, test_gpu_warp_edges.py): the case
table (source cameras, crafted / exact / small-source crop cameras, source images), the coordinate map of csrc/warp.hip restated in
numpy at a chosen precision, and the pixel classes the coverage checks count.  numpy only.

Source cameras 0 .. 3 and 4 .. 7 are recording 00's four Fisheye62 cameras at label frames 0 and 200; 8 is `axis_cam` (camera 0's
intrinsics and distortion at T = I); 9 is `far_cam` (axis_cam with its focal lengths x 2^19, so that coordinates leave every range
the samplers clamp to).  The MAIN table pairs them with 197 crop cameras: the 8 cameras gen_crop_cameras returns for
the two frames and both hands, each at focal x {1, 0.5, 0.25, 0.1} and turned by T @ Ry(deg), deg in {0, 30, 60, 90, 120, 180}
(192), three exact cases on axis_cam, and two straight-ahead crops on far_cam.  The SMALL tables pair the same source cameras, intrinsics scaled to an (h, w) image,
with the 8 cameras at the four focal factors, and at focal x 0.1 also turned by 60 degrees (40 per size), so that the image
boundary runs through the crops.

Measured on the CPU by test_warp_host.py (x86-64, 80-bit long double) over main + small tables, 357 cases:
  float64 restatement cast to float32 vs ref_camera.warp_map     0 mismatches of 6 580 224 entries
  float64 vs long double, relative to max(1, |coordinate|)       at most 7.96e-12 over the pixels in front (MAP_SPREAD)
  smallest |ez| / |e| outside the exact cases                    3.8e-7 (EZ_MARGIN asks for 1e-9)
  pixels per class (2 x 2 taps at the floor of the oracle's float32 map; see classify):
    size        inside  outside   left    right     top  bottom   behind   crops fully behind / fully inside
    480 x 636   765004   294597    136      498    1202    1536   752579   31 / 23
    1 x 1            0    36762    495   289277    6728  283044    42106    0 / 0
    2 x 3        60653    36762    495    91837    6728  191687    42106    0 / 0
    17 x 33     262823    40385    495     4427    3105   15299    42106    0 / 8
    64 x 48     275733    42612    447     3010     926    3806    42106    0 / 10
  Few pixels straddle a border of the full-size image: the Fisheye62 polynomial runs away just outside the calibrated field, so
  the map crosses a border's neighbourhood within a pixel or two.  The small sources are where the border classes get their numbers.
"""
import functools
import math

import numpy as np

from oracle import ref_camera, scenarios

CROP = 96
FRAMES = (0, 200)
FOCALS = (1.0, 0.5, 0.25, 0.1)
TURNS = (0, 30, 60, 90, 120, 180)
SMALL_VARIANTS = ((1.0, 0), (0.5, 0), (0.25, 0), (0.1, 0), (0.1, 60))
BIG = (480, 636)
SMALL_SIZES = ((1, 1), (2, 3), (17, 33), (64, 48))
CONTENTS = ("noise", "all255", "checker", "corners")
N_SRC = 10
AXIS_CAM, FAR_CAM = 8, 9

# Largest |float64 - long double| of the restated map over every in-front entry of every case, relative to max(1, |coordinate|),
# as test_warp_host.py measures it; MAP_SLACK = 8 x that (an FMA contraction or a device atan2 / sqrt a few ulp off the correctly
# rounded value each move a float64 chain by no more than the long-double chain differs from it).  A property of the reference
# arithmetic on the case table, never of the GPU's output.
MAP_SPREAD = 8.0e-12    # measured: 7.960e-12
MAP_SLACK = 8 * MAP_SPREAD
# no in-front / behind decision of a non-exact case may hang on rounding: |ez| / |e| stays above this
EZ_MARGIN = 1e-9


# ----------------------------------------------------------------------------- cameras
def _rec00_cameras(lab, fi):
    names = ("ImageSizeX", "ImageSizeY", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "k5", "k6")
    return [ref_camera.camera_from_json(dict(zip(names, lab["cameras"][ci])) | {"DistortionModel": "FishEye62"},
                                        lab["camera_to_world_transforms"][fi, ci]) for ci in range(4)]


@functools.lru_cache(maxsize=None)
def source_cameras():
    """The 10 source cameras (480 x 636)."""
    lab = scenarios.labels()
    cams = [c for fi in FRAMES for c in _rec00_cameras(lab, fi)]
    cams.append(dict(cams[0], T=np.eye(4)))
    cams.append(dict(cams[AXIS_CAM], f=tuple(2.0 ** 19 * np.asarray(cams[0]["f"]))))
    return cams


def scaled_source_cameras(size):
    """The 10 source cameras with f and c scaled by (w / 636, h / 480) to an h x w image."""
    h, w = size
    s = np.array([w / BIG[1], h / BIG[0]])
    return [dict(c, w=w, h=h, f=tuple(np.asarray(c["f"]) * s), c=tuple(np.asarray(c["c"]) * s)) for c in source_cameras()]


@functools.lru_cache(maxsize=None)
def base_crops():
    """[(crop camera, source index)] x 8: what gen_crop_cameras returns for both frames and both hands (right hands give the
    x-mirrored cameras)."""
    lab, hm, cams = scenarios.labels(), scenarios.hand_model_mm(), source_cameras()
    out = []
    for f, fi in enumerate(FRAMES):
        for hand in (0, 1):
            cc = ref_camera.gen_crop_cameras(cams[4 * f:4 * f + 4], lab["camera_angles"], hm, lab["joint_angles"][fi, hand],
                                             lab["wrist_transforms"][fi, hand], hand)
            out += [(crop, 4 * f + ci) for ci, crop in cc.items()]
    assert len(out) == 8
    return out


def _ry(deg):
    a = math.radians(deg)
    r = np.eye(4)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    return r


def _vary(crop, focal, deg):
    return dict(crop, f=tuple(focal * np.asarray(crop["f"])), T=np.asarray(crop["T"], np.float64) @ _ry(deg))


def _exact_crop(rot, focal=100.0):
    t = np.eye(4)
    t[:3, :3] = np.array(rot, np.float64)
    return {"w": CROP, "h": CROP, "f": (focal, focal), "c": (48.0, 48.0), "k": None, "T": t}


EXACT = {"identity": [[1, 0, 0], [0, 1, 0], [0, 0, 1]],           # pixel (48, 48) on the source axis: r == 0
         "backwards": [[-1, 0, 0], [0, 1, 0], [0, 0, -1]],        # pixel (48, 48) looks exactly backwards
         "quarter_turn": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]}      # pixel (48, 48): ez == 0, theta == pi / 2


class Case:
    def __init__(self, name, crop, src, exact=False):
        self.name, self.crop, self.src, self.exact = name, crop, src, exact


@functools.lru_cache(maxsize=None)
def main_cases():
    """The 197 cases on the 480 x 636 source cameras: 192 crafted, the three exact ones, then the two on far_cam (at crop focal
    10 000 the map climbs through 32768 px to about 6e5 px; at 100 through 1e6 px, where the float sampler clamps, to about 6e7 px,
    past the 1e9 / 32 px at which the integer sampler saturates)."""
    out = [Case(f"b{b}.f{focal}.r{deg}", _vary(crop, focal, deg), si)
           for b, (crop, si) in enumerate(base_crops()) for focal in FOCALS for deg in TURNS]
    out += [Case(name, _exact_crop(rot), AXIS_CAM, exact=True) for name, rot in EXACT.items()]
    out += [Case(f"far.{focal}", _exact_crop(EXACT["identity"], focal), FAR_CAM) for focal in (1.0e4, 1.0e2)]
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """The 40 cases of a small source: every base crop at the four focal factors, and at focal x 0.1 turned by 60 degrees (`src`
    indexes scaled_source_cameras(size)).  The turned ones are the crops that reach the LEFT border: the Fisheye62 polynomial
    runs away just outside the calibrated field, so the map crosses a border's neighbourhood within a pixel or two and only few
    pixels straddle a border at all."""
    return [Case(f"b{b}.f{focal}.r{deg}", _vary(crop, focal, deg), si)
            for b, (crop, si) in enumerate(base_crops()) for focal, deg in SMALL_VARIANTS]


def tables():
    """[(size, source cameras, cases)]: the main table first, then one per small size."""
    return [(BIG, source_cameras(), main_cases())] + [(s, scaled_source_cameras(s), small_cases()) for s in SMALL_SIZES]


def ordinary_cases():
    """Main-table indices of the 8 unvaried crops (most of them fully inside the source image)."""
    return [i for i, c in enumerate(main_cases()) if c.name.endswith(".f1.0.r0")]


def behind_cases():
    """Main-table indices of the 8 crops turned by 180 degrees at focal x 1 (every pixel behind the source camera)."""
    return [i for i, c in enumerate(main_cases()) if c.name.endswith(".f1.0.r180")]


# ----------------------------------------------------------------------------- source images
def source_images(size, content, n=N_SRC, seed=0):
    """[n, h, w] u8: "noise" n distinct uniform images; the others n copies of one image."""
    h, w = size
    if content == "noise":
        rng = np.random.default_rng([seed, h, w])
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if content == "all255":
        img = np.full((h, w), 255, np.uint8)
    elif content == "checker":                                  # period 1: the steepest gradient, any wrong weight shows
        img = (((np.arange(h)[:, None] + np.arange(w)[None]) & 1) * 255).astype(np.uint8)
    elif content == "corners":
        img = np.zeros((h, w), np.uint8)
        img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = 255
    else:
        raise ValueError(content)
    return np.ascontiguousarray(np.broadcast_to(img, (n, h, w)))


# ----------------------------------------------------------------------------- the map, restated
def restated_map(src_cam, crop_cam, dtype=np.float64):
    """csrc/warp.hip::warp_coords in numpy at `dtype` (float64 or np.longdouble), every sum written out in the kernel's order.
    Returns (m [96,96,2] in dtype with (-1, -1) behind, behind [96,96] bool, |ez| / |e| [96,96])."""
    d = dtype
    f, c, rc = np.asarray(crop_cam["f"], d), np.asarray(crop_cam["c"], d), np.asarray(crop_cam["T"], np.float64).astype(d)
    sf, sc_, rs = np.asarray(src_cam["f"], d), np.asarray(src_cam["c"], d), np.asarray(src_cam["T"], np.float64).astype(d)
    k1, k2, k3, k4, p1, p2, k5, k6 = (d(v) for v in src_cam["k"])
    py, px = np.meshgrid(np.arange(CROP).astype(d), np.arange(CROP).astype(d), indexing="ij")
    one, two = d(1), d(2)
    qx, qy = (px - c[0]) / f[0], (py - c[1]) / f[1]
    nrm = np.maximum(d(5.43e-20), np.sqrt(qx * qx + qy * qy + one))
    vx, vy, vz = qx / nrm, qy / nrm, one / nrm
    wx = rc[0, 0] * vx + rc[0, 1] * vy + rc[0, 2] * vz + rc[0, 3]
    wy = rc[1, 0] * vx + rc[1, 1] * vy + rc[1, 2] * vz + rc[1, 3]
    wz = rc[2, 0] * vx + rc[2, 1] * vy + rc[2, 2] * vz + rc[2, 3]
    dx, dy, dz = wx - rs[0, 3], wy - rs[1, 3], wz - rs[2, 3]
    ex = rs[0, 0] * dx + rs[1, 0] * dy + rs[2, 0] * dz
    ey = rs[0, 1] * dx + rs[1, 1] * dy + rs[2, 1] * dz
    ez = rs[0, 2] * dx + rs[1, 2] * dy + rs[2, 2] * dz
    r = np.sqrt(ex * ex + ey * ey)
    s = np.arctan2(r, ez) / np.maximum(r, d(2.0 ** -128))
    ux, uy = ex * s, ey * s
    pi2 = d(9.869604401089358)
    r2 = np.minimum(np.maximum(ux * ux + uy * uy, -pi2), pi2)
    r4 = r2 * r2
    r6 = r2 * r4
    radial = one + k1 * r2 + k2 * r4 + k3 * r6 + k4 * (r4 * r4) + k5 * (r4 * r6) + k6 * (r6 * r6)
    x, y = ux * radial, uy * radial
    x2, y2, xy = x * x, y * y, x * y
    rr = x2 + y2
    xd = x + (two * p2 * xy + p1 * (rr + two * x2))
    yd = y + (two * p1 * xy + p2 * (rr + two * y2))
    m = np.stack((xd * sf[0] + sc_[0], yd * sf[1] + sc_[1]), -1)
    behind = ez < 0
    m[behind] = -1
    cosz = np.abs(ez) / np.sqrt(ex * ex + ey * ey + ez * ez)
    return m, behind, cosz.astype(np.float64)


def oracle_maps(cams, cases):
    """ref_camera.warp_map of every case, [n,96,96,2] float32."""
    return np.stack([ref_camera.warp_map(cams[c.src], c.crop) for c in cases])


def restated_maps(cams, cases, dtype=np.float64):
    """(maps [n,96,96,2] dtype, behind [n,96,96], |ez| / |e| [n,96,96]) of every case."""
    m, b, z = zip(*(restated_map(cams[c.src], c.crop, dtype) for c in cases))
    return np.stack(m), np.stack(b), np.stack(z)


def ulp32(x):
    """Spacing of float32 at |x| (float64 in, float64 out)."""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def bracket32(x):
    """The two float32 neighbours lo <= x <= hi of float64 x (lo == hi where x is a float32)."""
    x = np.asarray(x, np.float64)
    n = x.astype(np.float32)
    lo = np.where(n.astype(np.float64) > x, np.nextafter(n, np.float32(-np.inf)), n)
    hi = np.where(n.astype(np.float64) < x, np.nextafter(n, np.float32(np.inf)), n)
    return lo.astype(np.float32), hi.astype(np.float32)


# ----------------------------------------------------------------------------- pixel classes
CLASSES = ("inside", "outside", "left", "right", "top", "bottom", "behind")


def classify(maps, behind, size):
    """{class: bool [n,96,96]} from float32 maps: the 2 x 2 taps at (floor x, floor y) of an h x w source.  "inside": all four
    taps in the image; "outside": none; "left" / "right" / "top" / "bottom": the tap pair straddles that border and at least one
    tap is in the image.  "behind" pixels (map (-1, -1)) are counted as behind only."""
    h, w = size
    ix = np.floor(maps[..., 0].astype(np.float64))
    iy = np.floor(maps[..., 1].astype(np.float64))
    x_in = [(ix + k >= 0) & (ix + k < w) for k in (0, 1)]
    y_in = [(iy + k >= 0) & (iy + k < h) for k in (0, 1)]
    any_x, any_y = x_in[0] | x_in[1], y_in[0] | y_in[1]
    front = ~behind
    return {"inside": front & x_in[0] & x_in[1] & y_in[0] & y_in[1],
            "outside": front & ~(any_x & any_y),
            "left": front & ~x_in[0] & x_in[1] & any_y,
            "right": front & x_in[0] & ~x_in[1] & any_y,
            "top": front & ~y_in[0] & y_in[1] & any_x,
            "bottom": front & y_in[0] & ~y_in[1] & any_x,
            "behind": behind}
