"""The yardstick of the mesh rasteriser (csrc/render.hip): the rules of ut_render_mesh (include/umetrack_hip.h) stated in
numpy, in float64 - and, to learn how far float32 arithmetic moves an edge or a depth, restated in float32.

Rules: a vertex goes through the crop camera in float64 (R^T (p - t), / z, * f + c); a triangle with a vertex at eye
z < 1e-4 is skipped whole; no culling (vertices 1 and 2 are exchanged where the screen area is negative; an area that is zero,
infinite or not a number covers nothing); with E_ab(p) = (xb - xa)(py - ya) - (yb - ya)(px - xa) a pixel centre (integer
coordinates) is covered when E_01, E_12, E_20 >= 0, a zero counting only on a top or left edge (yb - ya < 0, or yb == ya and
xb - xa > 0);
1 / z = w0 + (E_20 (w1 - w0) + E_01 (w2 - w0)) / area; the smallest depth wins, the smaller triangle index on equal depth;
shade = round(255 |n . c| / (|n| |c|)), n the face normal and c the centroid in eye space.

The float32 restatement rounds the projected (x, y, 1 / z) to float32 and evaluates everything after that in float32,
which is what the kernel holds in LDS and computes with.

DELTA_PX / EPS_MM: 4 x the largest disagreement between the two in edge distance / in depth on all 738 label poses of
recording_00 in their own crop cameras (measured on the CPU with float32_disagreement below; the figures are in
DESIGN.md "Rendered hand"): the factor 4 is the margin the mesh-normal test uses, for the same reason - the kernel may
associate differently from numpy.  tests/test_render_host.py re-measures a part of the poses and holds the constants to it.

Below the yardstick: lattice_cases(), small scenes on which every edge function is exact in fp32, so that the fill, tie and clip
rules can be compared on every pixel (tests/test_gpu_render_rules.py), and rasterise_int, the rules once more in int64 with the
mistakes a renderer could make as a switch."""
import numpy as np

SIZE = 96
NEAR = 1e-4
# measured: edge distance 5.28e-6 px, depth 3.44e-3 mm (float32 restatement vs float64, 738 poses, 1476 crops); x 4, rounded up
DELTA_PX = 2.2e-5
EPS_MM = 1.4e-2
MAX_EXCLUDED_SHARE = 0.005


def project(vertices, crop_row):
    """fp32 world vertices [V,3] through a crop_params row [24]: (eye [V,3], x [V], y [V], w = 1 / z [V], skip [V]), float64."""
    row = np.asarray(crop_row, np.float64)
    d = np.asarray(vertices).astype(np.float64) - row[13:16]
    eye = d @ row[4:13].reshape(3, 3)                     # R^T d
    skip = ~(eye[:, 2] >= NEAR)
    z = np.where(skip, 1.0, eye[:, 2])
    return eye, eye[:, 0] / z * row[0] + row[2], eye[:, 1] / z * row[1] + row[3], 1.0 / z, skip


def _windows(lo, hi, limit=10):
    """Triangles grouped by bounding-box extent so that one huge triangle does not widen every window."""
    ext = np.maximum(hi[0] - lo[0], hi[1] - lo[1]) + 1
    small = ext <= limit
    return [sel for sel in (np.nonzero(small)[0], np.nonzero(~small)[0]) if len(sel)]


def rasterise(vertices, triangles, crop_row, dtype=np.float64, delta=None, eps=None, bbox_from=None, keep=False):
    """One crop.  Returns a dict: depth f64 [96,96] (+inf background), tri i32 (-1), shade u8 (0), depth2 (the second nearest
    surface, +inf where there is none), covered (number of pixels with a surface); with delta / eps also `excluded`
    (bool [96,96]: centre within delta of an edge of a non-skipped triangle - looked for in the triangle's bounding box
    grown by one pixel; or the two nearest surfaces closer than eps in depth).  dtype float32: the restatement.  bbox_from: the
    result of a float64 call with keep=True, whose pixel windows are reused so that edge distances and depths can be
    compared entry by entry (`dist`, `z`, `inside`, all [entries])."""
    dt = np.dtype(dtype).type
    tris = np.asarray(triangles).astype(np.int64)
    eye, x64, y64, w64, skip = project(vertices, crop_row)
    x, y, w = x64.astype(dtype), y64.astype(dtype), w64.astype(dtype)
    valid = ~skip[tris].any(1)
    X, Y, W = x[tris], y[tris], w[tris]                                  # [T,3]
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    neg = area < 0
    for A in (X, Y, W):
        A[neg] = A[neg][:, [0, 2, 1]]
    area = np.where(neg, -area, area)
    valid &= np.isfinite(area) & (area != 0)
    if bbox_from is None:
        with np.errstate(invalid="ignore"):
            lo = np.stack([np.ceil(np.maximum(X.min(1), 0)), np.ceil(np.maximum(Y.min(1), 0))])
            hi = np.stack([np.floor(np.minimum(X.max(1), SIZE - 1)), np.floor(np.minimum(Y.max(1), SIZE - 1))])
        valid &= (lo[0] <= hi[0]) & (lo[1] <= hi[1])
        lo = np.where(valid, lo, 0).astype(np.int64)
        hi = np.where(valid, hi, 0).astype(np.int64)
    else:
        lo, hi, valid = bbox_from["lo"], bbox_from["hi"], bbox_from["valid"]     # the same entries, in the same order
    ids = np.nonzero(valid)[0]
    out_pix, out_z, out_tri, near, kept = [], [], [], [], {"dist": [], "z": [], "inside": []}
    for sel in _windows(lo[:, ids], hi[:, ids]):
        t = ids[sel]
        n = len(t)
        wx = int((hi[0, t] - lo[0, t]).max()) + 3                        # the box grown by one pixel on each side
        wy = int((hi[1, t] - lo[1, t]).max()) + 3
        px = (lo[0, t] - 1)[:, None, None] + np.arange(wx)[None, None, :] + np.zeros((1, wy, 1), np.int64)
        py = (lo[1, t] - 1)[:, None, None] + np.arange(wy)[None, :, None] + np.zeros((1, 1, wx), np.int64)
        grown = (px <= (hi[0, t] + 1)[:, None, None]) & (py <= (hi[1, t] + 1)[:, None, None]) & (px >= 0) & (py >= 0) & \
                (px < SIZE) & (py < SIZE)
        box = (px >= lo[0, t][:, None, None]) & (px <= hi[0, t][:, None, None]) & (py >= lo[1, t][:, None, None]) & \
              (py <= hi[1, t][:, None, None])
        fx, fy = px.astype(dtype), py.astype(dtype)
        g = lambda a, k: a[t, k][:, None, None]
        inside = box.copy()
        es, dist = [], []
        for a, b in ((0, 1), (1, 2), (2, 0)):
            dx, dy = g(X, b) - g(X, a), g(Y, b) - g(Y, a)
            e = dx * (fy - g(Y, a)) - dy * (fx - g(X, a))
            tl = (dy < 0) | ((dy == 0) & (dx > 0))
            inside &= (e > 0) | ((e == 0) & tl)
            es.append(e)
            # distance from the pixel centre to the edge (the segment): the edge function over the edge's length where the foot of
            # the perpendicular lies on the edge, else the distance to the nearer end
            dx64, dy64 = dx.astype(np.float64), dy.astype(np.float64)
            rx, ry = (fx - g(X, a)).astype(np.float64), (fy - g(Y, a)).astype(np.float64)
            len2 = np.maximum(dx64 ** 2 + dy64 ** 2, 1e-300)
            foot = (rx * dx64 + ry * dy64) / len2
            ends = np.sqrt(np.minimum(rx ** 2 + ry ** 2, (rx - dx64) ** 2 + (ry - dy64) ** 2))
            dist.append(np.where((foot >= 0) & (foot <= 1), np.abs(e.astype(np.float64)) / np.sqrt(len2), ends))
        e01, e12, e20 = es
        with np.errstate(divide="ignore", invalid="ignore"):
            iz = g(W, 0) + (e20 * (g(W, 1) - g(W, 0)) + e01 * (g(W, 2) - g(W, 0))) / area[t][:, None, None]
            z = dt(1) / iz
        inside &= (z > 0) & np.isfinite(z)
        assert z.dtype == np.dtype(dtype) and e01.dtype == np.dtype(dtype)
        sel_in = np.nonzero(inside)
        out_pix.append(py[sel_in] * SIZE + px[sel_in])
        out_z.append(z[sel_in].astype(np.float64))
        out_tri.append(np.broadcast_to(t[:, None, None], inside.shape)[sel_in])
        if delta is not None:
            close = grown & (np.minimum(np.minimum(dist[0], dist[1]), dist[2]) < delta)
            near.append((py[close] * SIZE + px[close]))
        if keep or bbox_from is not None:
            kept["dist"].append(np.stack(dist, -1)[grown])
            kept["z"].append(z.astype(np.float64)[grown])
            kept["inside"].append(inside[grown])
    pix = np.concatenate(out_pix) if out_pix else np.zeros(0, np.int64)
    zs = np.concatenate(out_z) if out_z else np.zeros(0)
    tr = np.concatenate(out_tri) if out_tri else np.zeros(0, np.int64)
    order = np.lexsort((tr, zs, pix))
    pix, zs, tr = pix[order], zs[order], tr[order]
    first = np.ones(len(pix), bool)
    first[1:] = pix[1:] != pix[:-1]
    second = np.zeros(len(pix), bool)
    second[1:] = first[:-1] & ~first[1:]
    depth = np.full(SIZE * SIZE, np.inf)
    depth2 = np.full(SIZE * SIZE, np.inf)
    tri = np.full(SIZE * SIZE, -1, np.int32)
    depth[pix[first]], tri[pix[first]] = zs[first], tr[first]
    depth2[pix[second]] = zs[second]
    # flat headlight shading per triangle, float64, from the eye-space vertices themselves
    P = eye[tris]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    cen = P.mean(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cosine = np.abs((nrm * cen).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(cen, axis=1))
    level = np.rint(255.0 * np.clip(np.nan_to_num(cosine), 0, 1)).astype(np.uint8)
    shade = np.where(tri >= 0, level[np.maximum(tri, 0)], 0).astype(np.uint8)
    res = {"depth": depth.reshape(SIZE, SIZE), "tri": tri.reshape(SIZE, SIZE), "shade": shade.reshape(SIZE, SIZE),
           "depth2": depth2.reshape(SIZE, SIZE), "covered": int(first.sum())}
    if delta is not None:
        ex = np.zeros(SIZE * SIZE, bool)
        if near:
            ex[np.concatenate(near)] = True
        if eps is not None:
            with np.errstate(invalid="ignore"):
                ex |= (depth2 - depth) < eps                             # inf - inf = nan compares false
        res["excluded"] = ex.reshape(SIZE, SIZE)
    if keep:
        res.update(lo=lo, hi=hi, valid=valid)
    if keep or bbox_from is not None:
        res.update({k: (np.concatenate(v) if v else np.zeros(0)) for k, v in kept.items()})
    return res


def float32_disagreement(vertices, triangles, crop_row):
    """(largest |edge distance float32 - float64| in px over every (pixel, edge) of the grown boxes, largest |depth float32 -
    float64| in mm over the entries both cover, the float64 result)."""
    with np.errstate(invalid="ignore"):
        r64 = rasterise(vertices, triangles, crop_row, np.float64, keep=True)
        r32 = rasterise(vertices, triangles, crop_row, np.float32, bbox_from=r64)
    assert r32["dist"].shape == r64["dist"].shape
    d_edge = float(np.abs(r32["dist"] - r64["dist"]).max()) if r64["dist"].size else 0.0
    both = r32["inside"] & r64["inside"]
    d_depth = float(np.abs(r32["z"][both] - r64["z"][both]).max()) if both.any() else 0.0
    return d_edge, d_depth, r64


def hand_case():
    """A scene small enough to work out by hand (tests/test_render_host.py): camera at the origin looking along +z, f = 128,
    c = 0.  Triangle 0: (0,0) (8,0) (0,8) px at z = 128.  Triangle 1: (2,2) z = 64, (10,2) z = 128, (2,10) z = 64.
    Triangle 2 has a vertex behind the camera.  Triangle 3 repeats triangle 0."""
    v = np.float32([[0, 0, 128], [8, 0, 128], [0, 8, 128], [1, 1, 64], [10, 2, 128], [1, 5, 64],
                    [0, 0, 128], [64, 64, 128], [0, 50, -10]])
    t = np.int32([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 1, 2]])
    row = np.zeros(24)
    row[0:2] = 128.0
    row[4:13] = np.eye(3).reshape(-1)
    return v, t, row


def label_crops_host(lab, hm, pose_ids):
    """Crop cameras of label poses on the host (oracle.ref_camera, the oracle of ut_gen_crop_cameras): a list of
    (pose id = frame * 2 + hand, [crop_params rows]) for the poses that have a view."""
    from absolutetrack_amd import geometry
    from oracle import ref_camera
    fields = ("ImageSizeX", "ImageSizeY", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "k5", "k6")
    out = []
    for pid in pose_ids:
        f, h = divmod(int(pid), 2)
        if lab["hand_confidences"][f, h] < 0.5:
            continue
        cams = []
        for ci in range(lab["cameras"].shape[0]):
            js = dict(zip(fields, lab["cameras"][ci]))
            js["DistortionModel"] = "FishEye62"
            cams.append(ref_camera.camera_from_json(js, lab["camera_to_world_transforms"][f, ci]))
        cc = ref_camera.gen_crop_cameras(cams, lab["camera_angles"], hm, lab["joint_angles"][f, h], lab["wrist_transforms"][f, h], h)
        rows = [geometry.pack_crop_camera(c["f"], c["c"], c["T"]) for c in cc.values()]
        if rows:
            out.append((int(pid), rows))
    return out


# ----------------------------------------------------------------------------- exact geometry: lattice cases
# Camera fx = fy = 128, R = I (or diag(-1, 1, 1)), t = 0, (cx, cy) on the quarter-pixel lattice; world vertices
# ((x - cx) z / 128, (y - cy) z / 128, z) with the screen (x, y) on the quarter-pixel lattice and z such that the products are
# fp32 numbers.  Then ex / ez = (x - cx) / 128 is representable, so the fp64 division, the multiplication by 128 and the
# addition of cx are all exact: the projection returns (x, y) itself.  In units of a quarter pixel a coordinate difference
# below 512 px is an integer below 2^11, an edge product an integer below 2^22 and the difference of two an integer below 2^23:
# every edge function and area is exact in fp32 (24 bits), and so coverage, the top-left decision and ownership are the same
# in integer arithmetic, in float64 and in the kernel's float32.  On the integer lattice the limit is 2048 px.  No pixel of
# these cases needs excluding.
LATTICE_LIMIT_QUARTER, LATTICE_LIMIT_INTEGER = 512, 2048
RENDER_MAX_VERTICES = 2368                                 # UT_RENDER_MAX_VERTICES
NEAR_F32 = np.float32(1e-4)                                # 9.99999974737875e-05: below 1e-4 as a double
NEAR_KEPT = np.nextafter(NEAR_F32, np.float32(1))          # the first float32 that is not


def lattice_row(cx=0.0, cy=0.0, mirror=False):
    """A crop_params row of the lattice camera; mirror: world -> eye is diag(-1, 1, 1), the crop camera of a right hand."""
    row = np.zeros(24)
    row[0:2] = 128.0
    row[2:4] = cx, cy
    row[4:13] = np.diag([-1.0 if mirror else 1.0, 1.0, 1.0]).reshape(-1)
    return row


def lattice_vertices(xy, z, row=None):
    """fp32 world vertices [n,3] that the camera `row` (default lattice_row()) sees at the screen points xy [n,2] px, depth z
    (scalar or [n]).  Refuses a point whose world coordinates are not fp32 numbers."""
    row = lattice_row() if row is None else row
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, np.float64), xy.shape[:1])
    v = np.stack([(xy[:, 0] - row[2]) * z / 128.0 * row[4], (xy[:, 1] - row[3]) * z / 128.0, z], 1)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "not representable in fp32"
    return v32


def _sheet(rng, n, spacing, origin, jitter):
    """A grid of n x n vertices `spacing` px apart from `origin`, each moved by a multiple of a quarter pixel up to `jitter` in
    x and in y; two triangles per cell, the diagonal, the winding and the first vertex of each drawn at random, the triangle
    order shuffled.  jitter < spacing / 4 keeps every triangle's orientation (the cross product of two jittered edges stays
    above (spacing - 2 jitter)^2 - (2 jitter)^2 > 0), so the sheet stays a triangulation: a pixel inside has one owner.
    Returns (screen xy [n*n,2], triangles [2(n-1)^2,3])."""
    gy, gx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xy = np.stack([gx, gy], -1).reshape(-1, 2) * float(spacing) + np.asarray(origin, np.float64)
    if jitter:
        k = int(round(jitter * 4))
        assert 4 * jitter == k and 4 * jitter < spacing
        xy = xy + rng.integers(-k, k + 1, xy.shape) / 4.0
    tris = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            pair = ((a, b, c), (b, d, c)) if rng.integers(2) else ((a, b, d), (a, d, c))
            for t in pair:
                t = np.roll(t, int(rng.integers(3)))
                tris.append(t[::-1] if rng.integers(2) else t)
    tris = np.int32(tris)
    return xy, tris[rng.permutation(len(tris))]


def _case(name, vertices, triangles, crop_rows, sample_range, on_lattice=None, **extra):
    vertices = np.ascontiguousarray(vertices, np.float32)
    vertices = vertices[None] if vertices.ndim == 2 else vertices
    lat = np.ones(vertices.shape[:2], bool) if on_lattice is None else np.broadcast_to(on_lattice, vertices.shape[:2]).copy()
    return dict(name=name, vertices=vertices, triangles=np.ascontiguousarray(triangles, np.int32),
                crop_rows=np.ascontiguousarray(np.asarray(crop_rows, np.float64).reshape(-1, 24)),
                sample_range=np.asarray(sample_range, np.int64).reshape(-1, 2), on_lattice=lat, **extra)


def _soup(rng, shapes, flip=True):
    """Separate triangles from (three screen points, z) entries: (xy [3n,2], z [3n], triangles [n,3]), windings at random."""
    xy = np.float64([p for pts, _ in shapes for p in pts])
    z = np.float64([zz for _, zs in shapes for zz in np.broadcast_to(zs, 3)])
    tris = np.arange(3 * len(shapes)).reshape(-1, 3)
    if flip:
        sel = rng.integers(0, 2, len(shapes)).astype(bool)
        tris[sel] = tris[sel][:, ::-1]
    return xy, z, tris.astype(np.int32)


SHEET_Z = 128.0


def _sheet_integer(rng):
    return _sheet(rng, 15, 8, (-8, -8), 0)


def _sheet_jitter(rng):
    return _sheet(rng, 15, 8, (-8, -8), 1.0)


def lattice_cases():
    """The named cases of tests/test_render_host.py and tests/test_gpu_render_rules.py, an ordered dict name -> case.  A case:
    vertices f32 [P,V,3], triangles i32 [T,3], crop_rows f64 [N,24], sample_range i64 [P,2], on_lattice bool [P,V] (the
    vertices whose projection is claimed to be exact), and what the case's own test needs.  Seeded; nothing is read."""
    cases = {}

    def add(c):
        cases[c["name"]] = c
    plain = lattice_row()
    # the scene worked out by hand in test_render_host.py
    v, t, row = hand_case()
    add(_case("hand_case", v, t, [row], [[0, 1]], on_lattice=rasterisable(v)))
    # 8-px sheets over [-8, 104]^2: every pixel has one owner
    xy, t = _sheet_integer(np.random.default_rng(11))
    add(_case("sheet_integer", lattice_vertices(xy, SHEET_Z), t, [plain], [[0, 1]], single_owner=True))
    xy, t = _sheet_jitter(np.random.default_rng(12))
    add(_case("sheet_jitter", lattice_vertices(xy, SHEET_Z), t, [plain], [[0, 1]], single_owner=True))
    # 48 x 48 vertices 2 px apart, x from -30 to 64 and y from -10 to 84: across rows 47 / 48, out of the crop on the left and at
    # the top, ending inside it on the right and at the bottom; padded with unused vertices to the cap
    xy, t = _sheet(np.random.default_rng(13), 48, 2, (-30, -10), 0.25)
    v = np.zeros((RENDER_MAX_VERTICES, 3), np.float32)
    v[:len(xy)] = lattice_vertices(xy, SHEET_Z)
    assert len(t) == 4418 and len(xy) == 2304
    add(_case("sheet_dense", v, t, [plain], [[0, 1]], on_lattice=np.arange(RENDER_MAX_VERTICES) < len(xy)))
    # the seam of the two 48-row passes
    rng = np.random.default_rng(14)
    xy, z, t = _soup(rng, [
        (((2, 48), (20, 48), (11, 60)), 128), (((2, 48), (20, 48), (11, 36)), 128),        # a horizontal edge on y = 48 from below, above
        (((24, 47), (40, 47), (32, 30)), 128), (((24, 47), (40, 47), (32, 58)), 128),      # on y = 47
        (((44, 47.5), (60, 47.5), (52, 40)), 128), (((44, 47.5), (60, 47.5), (52, 56)), 128),   # on y = 47.5
        (((64, 40), (90, 48.25), (66, 56)), 128),                                          # rows 40 .. 56
        (((68, 47), (88, 48), (72, 52)), 64), (((4, 70), (30, 47), (30, 48)), 64),         # vertices on pixel centres of rows 47, 48
        (((0, 44), (96, 47), (0, 52)), 256)])                                              # behind them all, across the seam
    add(_case("seam", lattice_vertices(xy, z), t, [plain], [[0, 1]]))
    # the crop's borders
    xy, z, t = _soup(rng, [
        (((0, 0), (10, 0), (0, 10)), 128), (((95, 0), (95, 10), (85, 0)), 128), (((96, 20), (96, 30), (86, 20)), 128),
        (((-0.25, 40), (10, 40), (-0.25, 50)), 128), (((95.25, 40), (95.25, 50), (85, 40)), 128),
        (((20, 95), (30, 95), (20, 85)), 128), (((40, 96), (50, 96), (40, 86)), 128), (((60, 95.25), (70, 95.25), (60, 85)), 128),
        (((60, -0.25), (70, -0.25), (60, 10)), 128), (((0, 95), (0, 60), (10, 95)), 128), (((95, 95), (95, 80), (80, 95)), 128),
        (((-30, 10), (-10, 10), (-20, 30)), 64), (((100, 10), (120, 10), (110, 30)), 64),  # wholly left, right,
        (((10, -30), (30, -30), (20, -10)), 64), (((10, 100), (30, 100), (20, 120)), 64),  # above, below
        (((-0.75, 10), (-0.25, 30), (-0.5, 50)), 64), (((95.25, 10), (95.75, 30), (95.5, 50)), 64),   # slivers outside by a quarter
        (((10.25, 60.25), (30.75, 60.5), (10.25, 60.75)), 64), (((50.25, 55), (50.75, 75), (50.5, 55.25)), 64),   # between centres
        (((-1000, -200), (1000, -200), (0, 1000)), 256)])                                  # integer lattice, the whole crop
    add(_case("borders", lattice_vertices(xy, z), t, [plain], [[0, 1]], n_nothing=(11, 19)))
    # zero area in front of a sheet: collinear vertices, (a, a, b), (a, a, a)
    xy, t = _sheet_integer(np.random.default_rng(11))
    n0 = len(xy)
    xy = np.concatenate([xy, np.float64([(10, 10), (20, 20), (40, 40), (50.25, 7.5)])])
    z = np.concatenate([np.full(n0, SHEET_Z), np.full(4, 64.0)])
    t = np.concatenate([t, np.int32([(n0, n0 + 1, n0 + 2), (n0 + 2, n0, n0 + 1), (n0, n0, n0 + 3), (n0 + 3, n0, n0), (n0 + 3, n0 + 3, n0 + 3),
                                     (5, 5, 5), (7, 100, 7)])])
    add(_case("degenerate", lattice_vertices(xy, z), t, [plain], [[0, 1]], same_as="sheet_integer"))
    # depth ties: index 5 = index 4000; 6 and 7 coplanar and overlapping; 3000 nearer than 10
    shapes = {5: (((4, 4), (40, 4), (4, 40)), 128), 4000: (((4, 40), (40, 4), (4, 4)), 128),
              7: (((50, 4), (90, 4), (50, 44)), 128), 6: (((60, 50), (60, 10), (94, 10)), 128),
              10: (((4, 50), (44, 50), (4, 90)), 128), 3000: (((10, 76), (10, 56), (30, 56)), 64),
              20: (((50, 52), (92, 52), (92, 92)), 256), 2999: (((92.5, 92), (50.5, 52), (92.5, 52)), 256)}
    xy, z, small = _soup(rng, list(shapes.values()), flip=False)
    t = np.zeros((4001, 3), np.int32)                        # the rest: (0, 0, 0), which covers nothing
    t[list(shapes)] = small
    add(_case("ties", lattice_vertices(xy, z), t, [plain], [[0, 1]]))
    # mirrored cameras, and one pose in two crops of one call
    xy, t = _sheet_jitter(np.random.default_rng(12))
    v = lattice_vertices(xy, SHEET_Z)
    add(_case("mirrored", np.stack([v, v]), t, [plain, lattice_row(95.0, 0.0, True), lattice_row(0.25, 0.25), lattice_row(94.75, 0.5, True)],
              [[0, 2], [2, 4]], single_owner=True))
    v, t, row = hand_case()
    row_m = lattice_row(20.0, 0.0, True)
    add(_case("mirrored_hand", v, t, [row, row_m], [[0, 2]], on_lattice=rasterisable(v)))
    # two sloped sheets whose 1 / z cross on the screen line x = 47.5; pose 1: 96 for 128, which is no power of two
    pts_a, pts_b = ((-16, -16), (240, -16), (-16, 240)), ((-145, -16), (111, -16), (-145, 240))
    poses = []
    for far in (128.0, 96.0):
        xy, z, t = _soup(rng, [(pts_a, (far, 64, far)), (pts_b, (64, far, 64))], flip=False)
        poses.append(lattice_vertices(xy, z))
    add(_case("sloped", np.stack(poses), t, [plain, plain], [[0, 1], [1, 2]]))
    # the near plane, camera centre (48, 48): triangle 3 at the first float32 above 1e-4 is kept and hides the backdrop where
    # x + y < 96; 0 has a vertex at float32(1e-4), 1 at z = 0, 2 at z < 0: each would hide triangle 3 if it were drawn
    row = lattice_row(48.0, 48.0)
    k = np.float64(NEAR_KEPT)
    tri_k = np.float64([(-k, -k, k), (k, -k, k), (-k, k, k)])
    v = [tri_k.copy(), tri_k.copy(), tri_k.copy(), tri_k]
    v[0][0] = (-np.float64(NEAR_F32), -np.float64(NEAR_F32), NEAR_F32)
    v[1][1] = (k, -k, 0.0)
    v[2][2] = (-k, k, -k)
    back = lattice_vertices([(-16, -16), (112, -16), (-16, 112), (112, 112)], SHEET_Z, row)
    v = np.concatenate([np.concatenate(v).astype(np.float32), back])
    t = np.int32([(0, 1, 2), (3, 5, 4), (6, 7, 8), (9, 11, 10), (12, 13, 15), (12, 15, 14)])
    add(_case("near", v, t, [row], [[0, 1]], on_lattice=np.arange(16) >= 9))
    # unusual float values in front of, behind and without a full sheet; pose 0 is the bare sheet (the others behind the eye)
    add(_hostile())
    # three poses of one mesh in one call, the middle one unseen
    rng = np.random.default_rng(15)
    poses = []
    for _ in range(3):
        xy, t = _sheet(np.random.default_rng(16), 15, 8, (-8, -8), 0)
        poses.append(lattice_vertices(xy + rng.integers(-4, 5, xy.shape) / 4.0, SHEET_Z))
    add(_case("batch", np.stack(poses), t, [plain, lattice_row(95.0, 0.0, True), lattice_row(0.25, 0.25)], [[0, 2], [2, 2], [2, 3]],
              single_owner=True))
    return cases


# The cases in which every drawn triangle has one z for its three vertices and that z is a power of two: 1 / z, the
# interpolation (w0 + 0 / area) and the reciprocal back are exact, so the float32 restatement's depth is float32(z) itself
# (tests/test_render_host.py holds the set to that).  Elsewhere the depth is rounded: hand_case / mirrored_hand (a sloped
# triangle), sloped, near (z = nextafter(1e-4), whose reciprocal is rounded).
EXACT_DEPTH_CASES = ("sheet_integer", "sheet_jitter", "sheet_dense", "seam", "borders", "degenerate", "ties", "mirrored", "batch")


def case_crops(case):
    """(pose, crop) for every crop the case's sample_range names, in order."""
    return [(p, c) for p, (r0, r1) in enumerate(case["sample_range"]) for c in range(r0, r1)]


def rasterisable(vertices):
    """The vertices in front of the lattice camera at the origin (the others are never projected)."""
    return np.asarray(vertices)[..., 2] >= NEAR


HOSTILE_POSES = ("bare", "sheet in front", "sheet behind", "sheet absent")


def _hostile():
    """A full sheet_integer (z = 128) and, appended, triangles with unusual values in the vertices tensor (every index in
    range).  The appended triangles per pose: behind the eye (bare); at z = 256 (sheet in front); at z = 64 (sheet behind);
    at z = 64 with the sheet behind the eye (absent).  In order: a NaN x, a NaN z, x = +inf, y = -inf, z = -inf, a world x of
    3e38 (its projection overflows fp32 at z = 64 and stays finite at z = 256, where the area then overflows), and a triangle
    whose vertices are fp32 numbers but whose fp32 area is not ((-1e20, -1e20) (3e20, -1e20) (-1e20, 3e20) px: 1.6e41: its edge
    functions overflow with it), and a thin one, (8,40) (1e38,41) (8,44) px, whose area 4e38 overflows while its edge functions
    stay finite over the crop - the one a kernel draws unless it looks at the area; last, an ordinary triangle (32,32) (64,32)
    (32,64), which must be drawn.  A vertex at z = +inf is left out: it projects to the camera
    centre with 1 / z = 0, which both the rules and the kernel draw, with a depth that crosses the sheet's on a curve."""
    xy, t = _sheet_integer(np.random.default_rng(11))
    sheet = lattice_vertices(xy, SHEET_Z)
    n0, nan, inf = len(sheet), np.nan, np.inf
    base = np.float64([(8, 8), (80, 16), (16, 80)])

    def hostile(zh):
        w = np.concatenate([base * zh / 128.0, np.full((3, 1), zh)], 1)
        out = [w.copy() for _ in range(9)]
        out[0][0, 0] = nan
        out[1][1, 2] = nan
        out[2][2, 0] = inf
        out[3][0, 1] = -inf
        out[4][1, 2] = -inf
        out[5][2, 0] = 3e38
        out[6][:, :2] = np.float64([(-1e20, -1e20), (3e20, -1e20), (-1e20, 3e20)]) * zh / 128.0
        out[7][:, :2] = np.float64([(8, 40), (1e38, 41), (8, 44)]) * zh / 128.0
        out[8][:, :2] = np.float64([(32, 32), (64, 32), (32, 64)]) * zh / 128.0
        return np.concatenate(out).astype(np.float32)
    behind_eye = np.tile(np.float32([[1, 2, -50]]), (27, 1))
    gone = sheet.copy()
    gone[:, 2] = -SHEET_Z
    poses = np.stack([np.concatenate(p) for p in ((sheet, behind_eye), (sheet, hostile(256.0)), (sheet, hostile(64.0)), (gone, hostile(64.0)))])
    extra = np.arange(27, dtype=np.int32).reshape(9, 3) + n0
    lat = np.zeros((4, n0 + 27), bool)
    lat[:3, :n0] = True
    return _case("hostile", poses, np.concatenate([t, extra]), [lattice_row()] * 4, [[0, 1], [1, 2], [2, 3], [3, 4]], on_lattice=lat,
                 n_sheet=len(t), nan_triangles=(len(t), len(t) + 1), overflow_triangles=(len(t) + 5, len(t) + 6, len(t) + 7),
                 plain_triangle=len(t) + 8)


# ----------------------------------------------------------------------------- the rules once more, in integers
RULES = ("top_left", "inclusive", "exclusive", "bottom_right", "top_left_before_exchange", "higher_index", "cull_negative")


def rasterise_int(vertices, triangles, crop_row, rule="top_left"):
    """An independent restatement on 4 x the screen coordinates in int64: coverage, the winding exchange, the top-left rule;
    ownership by (z, index) where every drawn triangle has one z for its three vertices.  For lattice cases only: the
    projected coordinates must be multiples of a quarter pixel (asserted for every triangle that is drawn).  Returns a dict:
    count i32 [96,96] (the number of triangles covering each centre) and tri i32 [96,96] (-1 background; None if a drawn
    triangle is not of constant z).  rule: "top_left" is the renderer's; the others are mistakes a renderer could make -
    every zero edge value counts / none does / zeros count on bottom and right edges / the top-left flags are taken before the
    vertices are exchanged and used after / the higher index wins a tie / triangles of negative area are culled."""
    assert rule in RULES
    eye, x, y, _, skip = project(vertices, crop_row)
    count = np.zeros((SIZE, SIZE), np.int32)
    best_z = np.full((SIZE, SIZE), np.inf)
    best_t = np.full((SIZE, SIZE), -1, np.int64)
    constant = True
    for t, (a, b, c) in enumerate(np.asarray(triangles).astype(np.int64)):
        if skip[a] or skip[b] or skip[c] or len({a, b, c}) < 3:
            continue
        fx, fy = x[[a, b, c]] * 4.0, y[[a, b, c]] * 4.0
        if not (np.isfinite(fx).all() and np.isfinite(fy).all()):
            continue
        assert (fx == np.rint(fx)).all() and (fy == np.rint(fy)).all() and np.abs(fx).max() < 2 ** 40 and np.abs(fy).max() < 2 ** 40
        qx, qy = [int(v) for v in fx], [int(v) for v in fy]
        area = (qx[1] - qx[0]) * (qy[2] - qy[0]) - (qy[1] - qy[0]) * (qx[2] - qx[0])
        if area == 0 or (rule == "cull_negative" and area < 0):
            continue
        flags_before = [_zero_counts(qx[j] - qx[i], qy[j] - qy[i], rule) for i, j in ((0, 1), (1, 2), (2, 0))]
        order = [0, 2, 1] if area < 0 else [0, 1, 2]
        qx, qy = [qx[i] for i in order], [qy[i] for i in order]
        x_lo, x_hi = max(-(-min(qx) // 4), 0), min(max(qx) // 4, SIZE - 1)
        y_lo, y_hi = max(-(-min(qy) // 4), 0), min(max(qy) // 4, SIZE - 1)
        if x_lo > x_hi or y_lo > y_hi:
            continue
        px = 4 * np.arange(x_lo, x_hi + 1, dtype=np.int64)[None, :]
        py = 4 * np.arange(y_lo, y_hi + 1, dtype=np.int64)[:, None]
        inside = np.ones((y_hi - y_lo + 1, x_hi - x_lo + 1), bool)
        for n, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
            dx, dy = qx[j] - qx[i], qy[j] - qy[i]
            e = dx * (py - qy[i]) - dy * (px - qx[i])
            zero = flags_before[n] if rule == "top_left_before_exchange" else _zero_counts(dx, dy, rule)
            inside &= (e > 0) | ((e == 0) & zero)
        z = eye[[a, b, c], 2]
        if not (z[0] == z[1] == z[2]):
            constant = False
        win = (slice(y_lo, y_hi + 1), slice(x_lo, x_hi + 1))
        count[win] += inside
        closer = inside & ((z[0] < best_z[win]) | ((z[0] == best_z[win]) & (rule == "higher_index")))   # t only grows
        best_z[win] = np.where(closer, z[0], best_z[win])
        best_t[win] = np.where(closer, t, best_t[win])
    return dict(count=count, tri=best_t.astype(np.int32) if constant else None)


def _zero_counts(dx, dy, rule):
    if rule == "inclusive":
        return True
    if rule == "exclusive":
        return False
    if rule == "bottom_right":
        return dy > 0 or (dy == 0 and dx < 0)
    return dy < 0 or (dy == 0 and dx > 0)


def on_edge_count(vertices, triangles, crop_row):
    """The number of pixel centres of the crop that lie exactly on an edge (the segment, ends included) of a drawn triangle of
    a lattice case - the pixels the fill rule decides."""
    _, x, y, _, skip = project(vertices, crop_row)
    hit = np.zeros((SIZE, SIZE), bool)
    px, py = 4 * np.arange(SIZE, dtype=np.int64)[None, :], 4 * np.arange(SIZE, dtype=np.int64)[:, None]
    for a, b, c in np.asarray(triangles).astype(np.int64):
        if skip[a] or skip[b] or skip[c] or not np.isfinite(x[[a, b, c]]).all() or not np.isfinite(y[[a, b, c]]).all():
            continue
        for i, j in ((a, b), (b, c), (c, a)):
            xi, yi, xj, yj = (int(v) for v in np.rint(4 * np.float64([x[i], y[i], x[j], y[j]])))
            if abs(xi) > 2 ** 40 or abs(xj) > 2 ** 40 or abs(yi) > 2 ** 40 or abs(yj) > 2 ** 40 or (xi, yi) == (xj, yj):
                continue
            e = (xj - xi) * (py - yi) - (yj - yi) * (px - xi)
            along = (px - xi) * (xj - xi) + (py - yi) * (yj - yi)
            hit |= (e == 0) & (along >= 0) & (along <= (xj - xi) ** 2 + (yj - yi) ** 2)
    return int(hit.sum())


def lattice_extents(case):
    """For every (pose, crop, triangle all of whose vertices are on_lattice and drawable): asserts that the projected
    coordinates are multiples of a quarter pixel, and returns the largest coordinate difference inside a triangle, in px,
    over (the triangles with a vertex off the integer lattice, those on it)."""
    worst = [0.0, 0.0]
    tris = case["triangles"].astype(np.int64)
    for p, (r0, r1) in enumerate(case["sample_range"]):
        for c in range(r0, r1):
            _, x, y, _, skip = project(case["vertices"][p], case["crop_rows"][c])
            ok = case["on_lattice"][p] & ~skip
            assert (4 * x[ok] == np.rint(4 * x[ok])).all() and (4 * y[ok] == np.rint(4 * y[ok])).all(), case["name"]
            sel = tris[ok[tris].all(1)]
            if not len(sel):
                continue
            X, Y = x[sel], y[sel]
            ext = np.maximum(X.max(1) - X.min(1), Y.max(1) - Y.min(1))
            integer = ((X == np.rint(X)) & (Y == np.rint(Y))).all(1)
            for k, m in enumerate((~integer, integer)):
                if m.any():
                    worst[k] = max(worst[k], float(ext[m].max()))
    return tuple(worst)
