#!/usr/bin/env python3
"""Golden-vector generator (TEST INFRASTRUCTURE ONLY; runs in the build container
where /root/reference is mounted - never on the GPU box).

    cd /root/repo && python oracle/gen_goldens.py

Imports the REFERENCE's own Python (lib.models.*, lib.common.{camera,crop,affine})
from /root/reference, drives it with the seeded synthetic weights/inputs of
absolutetrack_amd.synth, and writes small fixtures (inputs that cannot be
regenerated + expected outputs) under tests/golden/:

  model_known.npz / model_unknown.npz   reference UmeTrackModel outputs (rows a3-a10)
  geometry_rec00.npz                    reference crop cameras + warp coordinate maps (a1,a2)
  fk_user05.npz                         label poses + the reference's STORED gt_keypoints (a12)
  torch_data.npz                        reference lib.batched_dataset.data_transform crops + matrices (f2)
  metrics.npz                           reference load_eval._compute_metrics / metric_utils outputs (f4)
  *.torch.idx / *.torch.bin             files from the product's writer, verified readable by the reference's TorchIdx (f3)
  dropin_loader_rows.npz                what the reference's loader yields from them through the drop-in lib/ (8 b)
and the label data the bench/tests drive the path with:
  absolutetrack_amd/data/recording_00_labels.npz   (from sample_data/recording_00.json)

Not importable in this image, hence NOT run here: lib.common.hand_skinning /
lib.tracker.perspective_crop (pytorch3d), lib.tracker.tracker (cv2),
lib.tracker.video_pose_data (av).  No stand-ins are written for them.
"""
import json
import os
import sys

REF = "/root/reference"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from absolutetrack_amd import arch, formats, synth  # noqa: E402
from oracle import ref_camera, ref_fk, scenarios, stored_eval  # noqa: E402

# From here on `lib` must be the REFERENCE's package.  The reference's lib/ is a namespace package (no
# __init__.py) and the repo's drop-in lib/ is a regular one, which would win regardless of sys.path order:
# take the repo off the path (everything needed from it is already imported) and drop any cached `lib`.
sys.path[:] = [REF] + [p for p in sys.path if os.path.abspath(p or ".") != REPO]
for _m in [m for m in sys.modules if m == "lib" or m.startswith("lib.")]:
    del sys.modules[_m]

GOLD = os.path.join(REPO, "tests", "golden")
DATA = os.path.join(REPO, "absolutetrack_amd", "data")


# ----------------------------------------------------------------------------- reference model
def build_reference_model():
    import lib.models.feature_extractor as fe
    import lib.models.skeleton_encoder as se
    import lib.models.temporal as tem
    from lib.models.model_loader import _create_regressor
    from lib.models.model_opts import ModelOpts
    from lib.models.umetrack_model import UmeTrackModel
    assert fe.__file__.startswith(REF), fe.__file__
    mo = ModelOpts()
    f = fe.FeatureExtractor((96, 96), mo)
    model = UmeTrackModel(
        feature_extractor=f,
        temporal=tem.create_temporal_model(mo, f.output_feature_sizes),
        skeleton_encoder=se.SkeletonEncoder([mo.nSkeletonFeatureChannels, *f.output_feature_sizes]),
        regressor_k=_create_regressor(mo, f.output_feature_sizes, use_skel=True, predict_skel_scale=False),
        regressor_u=_create_regressor(mo, f.output_feature_sizes, use_skel=False, predict_skel_scale=True),
    )
    sd = {k: torch.from_numpy(v) for k, v in synth.synthetic_state_dict(0).items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    return model


def run_model_scenario(known: bool):
    from lib.models.umetrack_model import InputFrameData, InputFrameDesc, InputSkeletonData
    model = build_reference_model()
    taps = {}
    bb = model._feature_extractor._image_backbone
    hooks = [bb[0]._layers[0].register_forward_hook(lambda m, i, o: taps.__setitem__("stem", o)),
             bb[0]._layers[1].register_forward_hook(lambda m, i, o: taps.__setitem__("layer1", o)),
             bb[0]._layers[2].register_forward_hook(lambda m, i, o: taps.__setitem__("layer2", o)),
             bb[0]._layers[3].register_forward_hook(lambda m, i, o: taps.__setitem__("layer3", o)),
             bb[0]._layers[4].register_forward_hook(lambda m, i, o: taps.__setitem__("layer4", o)),
             bb[1].register_forward_hook(lambda m, i, o: taps.__setitem__("proj", o)),
             model._temporal.register_forward_hook(lambda m, i, o: None)]
    reg = model._regressor_k if known else model._regressor_u
    hooks.append(reg._pose_regression_layers.register_forward_hook(
        lambda m, i, o: taps.__setitem__("raw", o.flatten(1))))
    out = {}
    steps = scenarios.model_steps(known)
    skel = scenarios.skeleton_m()
    with torch.no_grad():
        for si, st in enumerate(steps):
            fd = InputFrameData(left_images=torch.from_numpy(st["images"]),
                                intrinsics=torch.from_numpy(st["intrinsics"]),
                                extrinsics_xf=torch.from_numpy(st["extrinsics"]))
            desc = InputFrameDesc(sample_range=torch.from_numpy(st["sample_range"]),
                                  memory_idx=torch.from_numpy(st["memory_idx"]),
                                  use_memory=torch.from_numpy(st["use_memory"]),
                                  hand_idx=torch.from_numpy(st["hand_idx"]))
            if known:
                sk = InputSkeletonData(joint_rotation_axes=torch.from_numpy(skel[0]),
                                       joint_rest_positions=torch.from_numpy(skel[1]))
                r = model.regress_pose_use_skeleton(fd, desc, sk)
            else:
                r = model.regress_pose_pred_skel_scale(fd, desc)
            p = f"s{si}."
            out[p + "joint_angles"] = r.joint_angles.numpy()
            out[p + "wrist_xfs"] = r.wrist_xfs.numpy()
            out[p + "sigmas"] = r.landmark_uncertainty_sigmas.numpy()
            if r.skel_scales is not None:
                out[p + "skel_scales"] = r.skel_scales.numpy()
            out[p + "raw"] = taps["raw"].numpy()
            out[p + "proj"] = taps["proj"].numpy()
            out[p + "mem_state"] = model._temporal._mem_features.numpy().copy()
            out[p + "prev_ext_state"] = model._temporal._prev_extrinsics.numpy().copy()
            if si == 0:   # early layers only once, spatially subsampled to keep the fixture small
                out["s0.stem_sub"] = taps["stem"][:, :, ::6, ::6].numpy()
                out["s0.layer1_sub"] = taps["layer1"][:, :, ::6, ::6].numpy()
                out["s0.layer2_sub"] = taps["layer2"][:, :, ::3, ::3].numpy()
                out["s0.layer3_sub"] = taps["layer3"][:, ::2, ::2, ::2].numpy()
                out["s0.layer4_sub"] = taps["layer4"][:, ::4].numpy()
    for h in hooks:
        h.remove()
    return out


# ----------------------------------------------------------------------------- labels / FK
HM_FIELDS = ("joint_rotation_axes", "joint_rest_positions", "landmark_rest_positions",
             "landmark_rest_bone_weights", "landmark_rest_bone_indices", "joint_limits")


def hand_model_arrays(hm: dict, prefix="hm."):
    return {prefix + k: np.asarray(hm[k], np.float32 if k != "landmark_rest_bone_indices" else np.int32)
            for k in HM_FIELDS}


def export_labels():
    d = json.load(open(os.path.join(REF, "sample_data", "recording_00.json")))
    cams = d["cameras"]
    names = ("ImageSizeX", "ImageSizeY", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "k5", "k6")
    assert all(c["DistortionModel"] == "FishEye62" for c in cams)
    out = {"cameras": np.array([[c[n] for n in names] for c in cams], np.float64),
           "camera_angles": np.asarray(d["camera_angles"], np.float64),
           "joint_angles": np.asarray(d["joint_angles"], np.float64),
           "wrist_transforms": np.asarray(d["wrist_transforms"], np.float64),
           "hand_confidences": np.asarray(d["hand_confidences"], np.float64),
           "camera_to_world_transforms": np.asarray(d["camera_to_world_transforms"], np.float64)}
    out.update(hand_model_arrays(d["hand_model"]))
    os.makedirs(DATA, exist_ok=True)
    np.savez_compressed(os.path.join(DATA, "recording_00_labels.npz"), **out)
    return d


def export_generic_hand_model():
    """dataset/generic_hand_model.json (the skeleton run_eval_unknown_skeleton.py:146-147 calibrates) without its mesh."""
    d = json.load(open(os.path.join(REF, "dataset", "generic_hand_model.json")))
    out = {k: np.asarray(v, np.int64 if k == "landmark_rest_bone_indices" else np.float32) for k, v in d.items()
           if not k.startswith("mesh_") and k != "dense_bone_weights"}
    np.savez_compressed(os.path.join(DATA, "generic_hand_model.npz"), **out)


def export_fk():
    out = {}
    for rec in ("00", "02", "11"):
        d = json.load(open(os.path.join(REF, "sample_data", "user05", f"recording_{rec}.json")))
        st = stored_eval.read_stored_eval(os.path.join(REF, "sample_data", "user05", f"recording_{rec}.npy"))
        sel = np.arange(0, len(d["joint_angles"]), 9)
        p = f"r{rec}."
        out[p + "joint_angles"] = np.asarray(d["joint_angles"], np.float64)[sel]
        out[p + "wrist_transforms"] = np.asarray(d["wrist_transforms"], np.float64)[sel]
        out[p + "hand_confidences"] = np.asarray(d["hand_confidences"], np.float64)[sel]
        out[p + "gt_keypoints"] = st["gt_keypoints"][:, sel]                 # [2,T,21,3] mm
        out[p + "valid_tracking"] = st["valid_tracking"][:, sel]
        out.update(hand_model_arrays(d["hand_model"], p + "hm."))
    np.savez_compressed(os.path.join(GOLD, "fk_user05.npz"), **out)


# ----------------------------------------------------------------------------- geometry
def export_geometry(labels: dict):
    import lib.common.camera as rcam
    import lib.common.crop as rcrop
    assert rcam.__file__.startswith(REF)
    hm = {k: np.asarray(labels["hand_model"][k]) for k in HM_FIELDS}
    frames = list(range(0, 369, 40))
    out = {"frames": np.array(frames)}
    for fi in frames:
        cams = []
        for ci, cj in enumerate(labels["cameras"]):
            c = rcam.read_camera_from_json(cj)
            cams.append(c.copy(camera_to_world_xf=np.asarray(labels["camera_to_world_transforms"][fi][ci])))
        for hand in (0, 1):
            ja = np.asarray(labels["joint_angles"][fi][hand])
            wx = np.asarray(labels["wrist_transforms"][fi][hand])
            # crop points: FK of (label pose, neutral pose, open pose) - FK itself is pinned separately
            lim = hm["joint_limits"].astype(np.float32)
            poses = (ja, lim[:, 0] * np.float32(0.5) + lim[:, 1] * np.float32(0.5), np.zeros(22, np.float32))
            pts = np.concatenate([ref_camera.landmarks_from_pose(hm, p, wx, hand) for p in poses], 0)
            lm = pts[:21]
            vis = []
            for c in cams:     # reference camera maths for the visibility count (perspective_crop.py:64-76)
                eye = c.world_to_eye(lm)
                win = c.eye_to_window(eye)
                vis.append(int(((win[..., 0] >= 0) & (win[..., 0] <= c.width - 1) & (win[..., 1] >= 0)
                                & (win[..., 1] <= c.height - 1) & (eye[..., 2] > 0)).sum()))
            key = f"f{fi}.h{hand}."
            out[key + "crop_points"] = pts
            out[key + "visible"] = np.array(vis)
            order = [i for i in range(4) if vis[i] >= 19]
            order.sort(reverse=True, key=lambda i: vis[i])
            order = sorted(order)[:2]
            out[key + "cams"] = np.array(order)
            for ci in order:
                crop = rcrop.gen_crop_parameters_from_points(
                    cams[ci], pts, (96, 96), mirror_img_x=(hand == 1),
                    camera_angle=labels["camera_angles"][ci], focal_multiplier=0.8)
                ck = key + f"c{ci}."
                out[ck + "f"] = np.asarray(crop.f, np.float64)
                out[ck + "c"] = np.asarray(crop.c, np.float64)
                out[ck + "T"] = np.asarray(crop.camera_to_world_xf, np.float64)
                out[ck + "K"] = np.asarray(crop.uv_to_window_matrix(), np.float64)
                # the coordinate map of lib/tracker/tracker.py:68-85, through the reference's camera methods
                px, py = np.meshgrid(np.arange(96), np.arange(96))
                dst = np.column_stack((px.flatten(), py.flatten()))
                seye = cams[ci].world_to_eye(crop.eye_to_world(crop.window_to_eye(dst)))
                swin = cams[ci].eye_to_window(seye)
                swin[seye[:, 2] < 0] = -1
                out[ck + "map_sub"] = swin.astype(np.float32).reshape(96, 96, 2)[::4, ::4]
    np.savez_compressed(os.path.join(GOLD, "geometry_rec00.npz"), **out)


# ----------------------------------------------------------------------------- torch_data batch path (row f2)
def export_torch_data():
    """Reference lib.batched_dataset.data_transform on the seeded sequences of scenarios.torch_data_case."""
    import lib.batched_dataset.data_transform as rdt
    assert rdt.__file__.startswith(REF), rdt.__file__
    out = {}
    for hand in (0, 1):
        c = scenarios.torch_data_case(hand)
        n_frames = c["images"].shape[0]
        res = np.empty((n_frames, 2, 4, 4), np.float32)
        for f in range(n_frames):
            _e, _k, res[f] = rdt._gen_crop_matrices(c["extrinsics"][f], c["intrinsics"][f], c["crop_points"][f], hand == 1,
                                                    (96, 96))
        img, ext, intr = rdt._perspective_crop_images(c["images"].astype(np.float32), c["extrinsics"], c["intrinsics"],
                                                      c["crop_points"], hand, (96, 96))
        key = f"h{hand}."
        out[key + "resample_xf"] = res
        out[key + "images"] = np.asarray(img, np.float32)
        out[key + "extrinsics_xf"] = ext
        out[key + "intrinsics"] = intr
        # The same reference functions on the same values held as float64: the look-at chain (six LAPACK inverses,
        # several GEMMs) then runs in double precision and is rounded to float32 once, at the stores into the
        # function's float32 result arrays.  The float32 run above differs from this one by the rounding of OpenBLAS's
        # sgesv / sgemm kernels, whose operation order depends on the kernel DYNAMIC_ARCH picks for the host CPU.
        res64 = np.empty((n_frames, 2, 4, 4), np.float32)
        ext64 = np.empty((n_frames, 2, 4, 4), np.float32)
        intr64 = np.empty((n_frames, 2, 3, 3), np.float32)
        for f in range(n_frames):
            ext64[f], intr64[f], res64[f] = rdt._gen_crop_matrices(
                c["extrinsics"][f].astype(np.float64), c["intrinsics"][f].astype(np.float64),
                c["crop_points"][f].astype(np.float64), hand == 1, (96, 96))
        out[key + "resample_xf_f64chain"] = res64
        out[key + "extrinsics_xf_f64chain"] = ext64
        out[key + "intrinsics_f64chain"] = intr64
    np.savez_compressed(os.path.join(GOLD, "torch_data.npz"), **out)


# ----------------------------------------------------------------------------- metrics (row f4)
def export_metrics():
    """Reference load_eval._compute_metrics + lib.common.metric_utils on the seeded eval-result arrays."""
    import lib.common.metric_utils as rmu
    import load_eval as rle
    assert rmu.__file__.startswith(REF) and rle.__file__.startswith(REF)
    c = scenarios.metrics_case()
    m = rle._compute_metrics(c["gt_keypoints"], c["tracked_keypoints"], c["valid_tracking"])
    pck = rmu.PCK_curve(m.keypoint_errors, rmu.PCK_THRESHOLDS) * 100.0
    per_hand = rmu.PCK_curve(np.linalg.norm(c["gt_keypoints"] - c["tracked_keypoints"], axis=-1), rmu.PCK_THRESHOLDS,
                             mask=np.repeat(c["valid_tracking"][..., None], 21, -1).astype(np.float64), axis=0)
    np.savez_compressed(os.path.join(GOLD, "metrics.npz"), keypoint_errors=m.keypoint_errors,
                        keypoint_accelerations=m.keypoint_accelerations,
                        gt_keypoint_accelerations=m.gt_keypoint_accelerations, pck=pck,
                        auc=np.float64(rmu.normalized_AUC(rmu.PCK_THRESHOLDS, pck)), pck_per_hand=per_hand,
                        auc_per_hand=rmu.normalized_AUC(rmu.PCK_THRESHOLDS, per_hand))


# ----------------------------------------------------------------------------- .torch.idx/.bin (row f3)
def export_idxbin():
    """Fixture files written by the product's writer; the REFERENCE's TorchIdx must parse them to the same data."""
    import lib.data_utils.idxbinfile as ridx
    assert ridx.__file__.startswith(REF)
    c = scenarios.idxbin_case()
    for name, frames in (("seq_mono", c["mono"]), ("seq_labels", c["labels"]), ("ragged_f32", c["ragged"])):
        path = os.path.join(GOLD, name + ".torch.idx")
        formats.write_torch_idx_bin(path, frames)
        ref = ridx.TorchIdx(path)
        assert len(ref) == len(frames)
        with open(ref.bin_path, "rb") as f:
            raw = f.read()
        # (the reference's read_bin() of a non-uniform file trips over its own map_dataset(range); go per frame)
        whole = ref.view_buffer(raw) if ref.shape is not None else None
        for i in range(len(frames)):
            got = whole[i] if whole is not None else ref.view_buffer_at(i, raw)
            if isinstance(frames[i], np.ndarray):
                assert np.array_equal(got, frames[i]) and got.dtype == frames[i].dtype, (name, i)
            else:
                assert got == frames[i], (name, i)
    assert ridx.TorchIdx(os.path.join(GOLD, "seq_mono.torch.idx")).shape == (3, 2, 2, 16, 24)
    # byte_offset / byte_offsets of the reference's TorchIdx on the three fixtures (uniform and ragged branch),
    # incl. the end == -1 and end == N + 1 forms its async reader uses (lib/data_utils/idxbinfile.py:196-231)
    offs = {}
    for name in ("seq_mono", "seq_labels", "ragged_f32"):
        ref = ridx.TorchIdx(os.path.join(GOLD, name + ".torch.idx"))
        n = len(ref)
        offs[name + ".n"] = np.int64(n)
        offs[name + ".to_minus1"] = np.asarray(ref.byte_offsets(0, -1)).astype(np.int64)
        offs[name + ".to_n_plus_1"] = np.asarray(ref.byte_offsets(0, n + 1)).astype(np.int64)
        offs[name + ".from1_minus1"] = np.asarray(ref.byte_offsets(1, -1)).astype(np.int64)
        offs[name + ".from1_to_n"] = np.asarray(ref.byte_offsets(1, n)).astype(np.int64)
        offs[name + ".single"] = np.asarray([ref.byte_offset(i) for i in list(range(n + 1)) + [-1]], np.int64)
    np.savez_compressed(os.path.join(GOLD, "idxbin_offsets.npz"), **offs)


# ----------------------------------------------------------------------------- drop-in loader chain (SURVEY 8 b)
def export_dropin_loader_rows():
    """The rows the reference's own loader chain (find_dataset -> AsyncToIterableDataset), running on top of this
    repo's served lib.data_utils.{fs,idxbinfile} (repo first on PYTHONPATH, the reference behind it), yields from the
    seq_mono / seq_labels fixtures: dropin_loader_rows.npz (n, mono<i>, lab<i> = msgpack of the labels).
    The reference's Sampler passes an argument to torch.utils.data.Sampler.__init__ that this torch no longer
    accepts, so a plain index range stands in."""
    import shutil
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        leaf = os.path.join(tmp, "torch_data", "real", "testing")
        os.makedirs(leaf)
        for field, src in (("mono", "seq_mono"), ("labels", "seq_labels")):
            for ext in (".torch.idx", ".torch.bin"):
                shutil.copy(os.path.join(GOLD, src + ext), os.path.join(leaf, field + ext))
        code = f"""
import numpy as np, msgpack
import lib.data_utils.fs as fs, lib.data_utils.idxbinfile as ib
assert fs.__file__.startswith({REPO!r}) and ib.__file__.startswith({REPO!r})
from lib.data_utils.async_dataset import AsyncToIterableDataset, find_dataset
from lib.data_utils.split import Split
d = find_dataset([{os.path.join(tmp, "torch_data", "real")!r}], ["mono", "labels"])[Split.TEST]
rows = list(AsyncToIterableDataset(d, range(len(d)), max_prefetch=4))
np.savez_compressed({os.path.join(GOLD, "dropin_loader_rows.npz")!r}, n=len(rows),
                    **{{f"mono{{i}}": np.asarray(r["mono"]) for i, r in enumerate(rows)}},
                    **{{f"lab{{i}}": np.frombuffer(msgpack.packb(r["labels"]), np.uint8) for i, r in enumerate(rows)}})
"""
        subprocess.run([sys.executable, "-c", code], check=True, cwd=tmp,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, REF])))


def main():
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(8)
    labels = export_labels()
    export_generic_hand_model()
    export_fk()
    export_geometry(labels)
    export_torch_data()
    export_metrics()
    export_idxbin()
    export_dropin_loader_rows()
    np.savez_compressed(os.path.join(GOLD, "model_known.npz"), **run_model_scenario(True))
    np.savez_compressed(os.path.join(GOLD, "model_unknown.npz"), **run_model_scenario(False))
    for f in sorted(os.listdir(GOLD)):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()
