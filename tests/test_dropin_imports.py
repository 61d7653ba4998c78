"""CPU tests of the drop-in module paths (SURVEY.md section 8 b): the `lib/` package here serves the hot-path modules
and lets every module it does not serve fall through to a reference checkout later on sys.path
(run_inference_torch_data.py:13-31 imports lib.data_utils.{async_dataset,dataset_util,split} next to the served ones).

The fall-through is tested with synthetic sibling trees; what the reference's loader chain yields through the served
modules is recorded under tests/golden/ (oracle/gen_goldens.py)."""
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, pythonpath, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath))
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd=cwd, capture_output=True,
                          text=True, timeout=300)


def test_unserved_modules_fall_through_to_a_sibling_lib_tree(tmp_path):
    # a "reference checkout": namespace packages (no __init__.py), one module we do not serve at each level and one
    # we do serve (must lose against this repo's)
    sib = tmp_path / "checkout"
    (sib / "lib" / "data_utils").mkdir(parents=True)
    (sib / "lib" / "extra_pkg").mkdir(parents=True)
    (sib / "lib" / "tracker").mkdir(parents=True)
    (sib / "lib" / "data_utils" / "extra_mod.py").write_text(
        "from lib.data_utils import fs\nfrom .idxbinfile import TorchIdx\nWHO = 'sibling'\n")
    (sib / "lib" / "extra_pkg" / "mod.py").write_text("WHO = 'sibling pkg'\n")
    (sib / "lib" / "data_utils" / "fs.py").write_text("WHO = 'shadowed'\n")
    (sib / "lib" / "tracker" / "tracker.py").write_text("WHO = 'shadowed'\n")
    r = _run("""
        import lib.data_utils.extra_mod as e, lib.extra_pkg.mod as m
        import lib.data_utils.fs as fs, lib.tracker.tracker as t, lib.data_utils.idxbinfile as ib
        import absolutetrack_amd.formats as f
        assert e.WHO == 'sibling' and m.WHO == 'sibling pkg'
        assert e.fs is fs and not hasattr(fs, 'WHO') and hasattr(fs, 'read_bytes')
        assert e.TorchIdx is f.TorchIdx is ib.TorchIdx
        assert hasattr(t, 'HandTracker') and not hasattr(t, 'WHO')
        print(e.__file__, '|', t.__file__)
        """, [ROOT, str(sib)], str(tmp_path))
    assert r.returncode == 0, r.stderr
    ext, trk = r.stdout.strip().split(" | ")
    assert ext.startswith(str(sib)) and trk.startswith(ROOT)
    # without the sibling on the path the unserved module is simply absent
    r = _run("import lib.data_utils.extra_mod", [ROOT], str(tmp_path))
    assert r.returncode != 0 and "ModuleNotFoundError" in r.stderr


# the modules lib/ leaves to a reference checkout behind it (lib/__init__.py)
UNSERVED = ("lib.data_utils.async_dataset", "lib.data_utils.async_utils", "lib.data_utils.nested_async",
            "lib.data_utils.dataset_util", "lib.data_utils.split")

# the Python surface the drop-in must present: SURVEY.md section 8 (b) "Python surface that must exist" and
# INTEGRATION.md section A (what the unserved loader modules take from idxbinfile / fs)
SURFACE = {
    "lib.models.model_loader": ["load_pretrained_model"],
    "lib.models.umetrack_model": ["UmeTrackModel", "InputFrameData", "InputFrameDesc", "InputSkeletonData"],
    "lib.models.regressor": ["RegressorOutput"],
    "lib.tracker.tracker": ["HandTracker", "HandTrackerOpts", "InputFrame", "ViewData"],
    "lib.tracker.perspective_crop": ["landmarks_from_hand_pose"],
    "lib.tracker.tracking_result": ["SingleHandPose", "TrackingResult"],
    "lib.tracker.video_pose_data": ["SyncedImagePoseStream", "_load_json", "load_hand_model_from_dict"],
    "lib.common.hand": ["HandModel", "NUM_HANDS", "NUM_LANDMARKS_PER_HAND", "scaled_hand_model", "mirrored_hand_model"],
    "lib.common.hand_skinning": ["skin_landmarks"],
    "lib.common.camera": ["CameraModel", "PinholePlaneCameraModel", "Fisheye62CameraModel", "read_camera_from_json"],
    "lib.common.metric_utils": [],
    "lib.data_utils": ["bundles", "fs"],
    "lib.batched_dataset.sample": [],
    "lib.batched_dataset.data_transform": ["ModelInput", "preprocess"],
    "lib.data_utils.idxbinfile": ["OBJECT_DTYPE", "RawField", "TorchIdx"],
    "lib.data_utils.fs": ["read_bytes", "aread_bytes"],
    # left to the checkout (the torch_data script's loader)
    "lib.data_utils.async_dataset": ["AsyncToIterableDataset", "find_dataset", "Sampler", "subsample"],
    "lib.data_utils.dataset_util": ["map_dataset"],
    "lib.data_utils.split": ["Split"],
}
METHODS = {
    ("lib.tracker.tracker", "HandTracker"): ["gen_crop_cameras", "track_frame", "track_frame_and_calibrate_scale",
                                             "reset_history"],
    ("lib.models.umetrack_model", "UmeTrackModel"): ["eval", "to", "getInputImageSizes", "regress_pose_use_skeleton",
                                                     "regress_pose_pred_skel_scale"],
    ("lib.data_utils.idxbinfile", "TorchIdx"): ["byte_offsets"],
}
# a stand-in loader module takes what it needs through the served modules, as the checkout's loader does
STAND_IN_LOADER = (
    "from lib.data_utils import fs, nested_async\n"
    "from .idxbinfile import OBJECT_DTYPE, RawField, TorchIdx\n"
    "from .split import Split\n"
    "NEEDS = (fs.read_bytes, fs.aread_bytes, TorchIdx.byte_offsets)\n")


def test_dropin_modules_resolve_with_a_checkout_behind(tmp_path):
    """`PYTHONPATH=<repo>:<checkout>`: every module lib/ serves imports and resolves to this repo; every (module, name)
    of the documented drop-in surface (SURFACE, METHODS) resolves - served names from this repo, the loader's from the
    checkout, which itself imports through the served fs / idxbinfile; preprocess / load_pretrained_model / TorchIdx
    are the hot path's own objects.  The checkout is a stand-in tree of namespace packages."""
    sib = tmp_path / "checkout"
    for mod in UNSERVED:
        f = sib.joinpath(*mod.split(".")).with_suffix(".py")
        f.parent.mkdir(parents=True, exist_ok=True)
        body = "".join(f"class {n}:\n    pass\n" for n in SURFACE.get(mod, []))
        f.write_text((STAND_IN_LOADER if mod.endswith(".async_dataset") else "") + body + "WHO = 'checkout'\n")
    served = sorted(os.path.relpath(os.path.join(d, f), ROOT)[:-3].replace(os.sep, ".").replace(".__init__", "")
                    for d, _, fs in os.walk(os.path.join(ROOT, "lib")) for f in fs if f.endswith(".py"))
    assert "lib.data_utils.fs" in served and "lib.models.model_loader" in served
    assert set(SURFACE) <= set(served) | set(UNSERVED)
    r = _run(f"""
        import importlib, types
        for name in {served!r}:
            m = importlib.import_module(name)
            assert m.__file__.startswith({ROOT!r}), (name, m.__file__)
        for name in {list(UNSERVED)!r}:
            m = importlib.import_module(name)
            assert m.__file__.startswith({str(sib)!r}) and m.WHO == 'checkout', (name, m.__file__)
        unserved = {list(UNSERVED)!r}
        missing = []
        for mod, names in {SURFACE!r}.items():
            m = importlib.import_module(mod)
            want = {str(sib)!r} if mod in unserved else {ROOT!r}
            assert m.__file__.startswith(want), (mod, m.__file__)
            for n in names:
                try:
                    exec(f"from {{mod}} import {{n}}", {{}})       # `from M import N`, submodules included
                except ImportError:
                    missing.append(f"{{mod}}.{{n}}")
                    continue
                o = getattr(m, n)
                if isinstance(o, types.ModuleType):
                    assert o.__file__.startswith({ROOT!r}), (mod, n, o.__file__)
        for (mod, n), attrs in {METHODS!r}.items():
            cls = getattr(importlib.import_module(mod), n)
            missing += [f"{{mod}}.{{n}}.{{a}}" for a in attrs if not hasattr(cls, a)]
        assert not missing, missing
        import lib.data_utils.async_dataset as ad, lib.data_utils.fs as fs
        assert ad.fs is fs and ad.NEEDS[0] is fs.read_bytes
        import lib.batched_dataset.data_transform as dt, lib.models.model_loader as ml, lib.data_utils.idxbinfile as ib
        import absolutetrack_amd.torch_data as td, absolutetrack_amd.model as m, absolutetrack_amd.formats as f
        assert dt.preprocess is td.preprocess and ml.load_pretrained_model is m.load_pretrained_model
        assert ib.TorchIdx is f.TorchIdx and ad.TorchIdx is f.TorchIdx
        print('ok')
        """, [ROOT, str(sib)], str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr


def test_reference_dataset_loader_reads_through_the_served_idxbinfile(golden_dir):
    """The reference's own loader chain (find_dataset -> AsyncToIterableDataset, run_inference_torch_data.py:143-171),
    run on top of the TorchIdx / fs served here, yields the same raw sequences as formats.read_sequence.  Its rows
    are recorded in tests/golden/dropin_loader_rows.npz by oracle/gen_goldens.py (export_dropin_loader_rows)."""
    import msgpack
    from absolutetrack_amd import formats
    got = np.load(os.path.join(golden_dir, "dropin_loader_rows.npz"))
    assert int(got["n"]) == 3
    for i in range(3):
        want = formats.read_sequence(os.path.join(golden_dir, "seq_mono.torch.idx"),
                                     os.path.join(golden_dir, "seq_labels.torch.idx"), i)
        assert np.array_equal(got[f"mono{i}"], want["mono"]) and got[f"mono{i}"].dtype == want["mono"].dtype
        assert msgpack.unpackb(got[f"lab{i}"].tobytes()) == want["labels"]
