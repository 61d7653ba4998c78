"""The yardstick of the mesh rasteriser (csrc/render.hip): the rules of ut_render_mesh (include/umetrack_hip.h) stated in
numpy, in float64 - and, to learn how far float32 arithmetic moves an edge or a depth, restated in float32.

Rules: a vertex goes through the crop camera in float64 (R^T (p - t), / z, * f + c); a triangle with a vertex at eye
z < 1e-4 is skipped whole; no culling (vertices 1 and 2 are exchanged where the screen area is negative; zero area covers
nothing); with E_ab(p) = (xb - xa)(py - ya) - (yb - ya)(px - xa) a pixel centre (integer coordinates) is covered when
E_01, E_12, E_20 >= 0, a zero counting only on a top or left edge (yb - ya < 0, or yb == ya and xb - xa > 0);
1 / z = w0 + (E_20 (w1 - w0) + E_01 (w2 - w0)) / area; the smallest depth wins, the smaller triangle index on equal depth;
shade = round(255 |n . c| / (|n| |c|)), n the face normal and c the centroid in eye space.

The float32 restatement rounds the projected (x, y, 1 / z) to float32 and evaluates everything after that in float32,
which is what the kernel holds in LDS and computes with.

DELTA_PX / EPS_MM: 4 x the largest disagreement between the two in edge distance / in depth on all 738 label poses of
recording_00 in their own crop cameras (measured on the CPU with float32_disagreement below; the figures are in
DESIGN.md "Rendered hand"): the factor 4 is the margin the mesh-normal test uses, for the same reason - the kernel may
associate differently from numpy.  tests/test_render_host.py re-measures a part of the poses and holds the constants to it."""
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
