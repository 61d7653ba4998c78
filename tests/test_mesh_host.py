"""CPU tests of the posed-mesh feature: the fixture, the float64 oracle the GPU tests compare with (pinned to the pinned
landmark oracle) and the C declarations."""
import os
import shutil
import subprocess

import numpy as np

import mesh_cases as mc
from oracle import ref_fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_sanity():
    for which in ("rec00", "generic"):
        v, t, w = mc.load_mesh(which)
        assert v.shape == (788, 3) and v.dtype == np.float32 and np.isfinite(v).all()
        assert t.shape == (1544, 3) and t.dtype == np.int32 and t.min() >= 0 and t.max() < v.shape[0]
        assert w.shape == (788, 17) and w.dtype == np.float32 and np.isfinite(w).all()
        assert (w != 0).sum(1).max() <= 3
        assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= 1e-6
        assert np.array_equal(np.unique(t), np.arange(v.shape[0]))          # every vertex is used
    assert np.array_equal(mc.load_mesh("rec00")[2], mc.load_mesh("generic")[2])
    assert np.abs(mc.load_mesh("rec00")[0] - mc.load_mesh("generic")[0]).max() > 1.0      # a user mesh, not the generic one


def test_float64_oracle_is_pinned_to_the_landmark_oracle(golden_dir):
    """The mesh oracle fed the 21 landmark rest positions with densified landmark weights is skin_landmarks: it must
    agree with oracle.ref_fk.skin_landmarks (float32, itself pinned to the reference's stored gt_keypoints within 1e-3 mm
    by test_oracle_pinning) on the fk_user05 poses, within that same 1e-3 mm."""
    g = np.load(os.path.join(golden_dir, "fk_user05.npz"))
    worst = 0.0
    for rec in ("00", "02", "11"):
        p = f"r{rec}."
        hm = mc.skeleton(g, p + "hm.")
        for hand in (0, 1):
            ja = g[p + "joint_angles"][:, hand]
            xf = g[p + "wrist_transforms"][:, hand].copy()
            if hand == 1:
                xf[:, :, 0] *= -1
            want = ref_fk.skin_landmarks(hm, ja.astype(np.float32), xf.astype(np.float32))
            got = mc.skin(hm, hm["landmark_rest_positions"], mc.dense_landmark_weights(hm), ja.astype(np.float32),
                          xf.astype(np.float32), dtype=np.float64)
            worst = max(worst, float(np.abs(got - want).max()))
            got32 = mc.skin(hm, hm["landmark_rest_positions"], mc.dense_landmark_weights(hm), ja.astype(np.float32),
                            xf.astype(np.float32), dtype=np.float32)
            assert got32.dtype == np.float32
            worst = max(worst, float(np.abs(got32 - want).max()))
            # the mirror flag of the oracle is the negated column
            raw = g[p + "wrist_transforms"][:, hand].astype(np.float32)
            via_flag = mc.skin(hm, hm["landmark_rest_positions"], mc.dense_landmark_weights(hm), ja.astype(np.float32), raw,
                               dtype=np.float64, mirror=np.full(len(ja), hand))
            assert np.array_equal(via_flag, got)
    print(f"float64 / float32 mesh oracle vs ref_fk.skin_landmarks: max {worst:.3e} mm")
    assert worst < 1e-3


def test_oracle_normals_point_out_of_the_rest_mesh():
    """Stored winding is counter-clockwise seen from outside: positive volume, and moving every vertex along its
    normal grows the volume."""
    v, t, w = mc.load_mesh("rec00")
    hm = {"joint_rotation_axes": np.tile(np.float32([1, 0, 0]), (22, 1)), "joint_rest_positions": np.zeros((22, 3), np.float32)}
    p, nrm = mc.skin(hm, v, w, np.zeros((1, 22)), np.eye(4)[None], triangles=t)
    np.testing.assert_allclose(p[0], v.astype(np.float64), atol=1e-9)
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=-1), 1.0, atol=1e-12)
    vol = mc.signed_volume(p, t)[0]
    assert vol > 1e5 and mc.signed_volume(p + nrm, t)[0] > vol


def test_header_declares_the_mesh_entries_in_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to check the C99 header"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "mesh_c99.c"), "-o", str(tmp_path / "mesh_c99.o")])


def test_library_exports_the_mesh_entries_and_rejects_on_the_host():
    """Argument and mesh validation happen before any device is touched, so the refusals can be checked here."""
    import ctypes
    from absolutetrack_amd import _native
    lib = _native.load_library()
    for name in ("ut_mesh_create", "ut_mesh_destroy", "ut_mesh_counts", "ut_skin_mesh"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    v, t, w = mc.load_mesh("rec00")

    def create(v, t, w):
        h = ctypes.c_void_p()
        rc = lib.ut_mesh_create(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], w.ctypes.data, 0, ctypes.byref(h))
        assert rc != 0 and not h.value
        return rc, lib.ut_last_error(None).decode()

    bad = w.copy(); bad[5, :5] = 0.2
    assert create(v, t, bad) == (-4, "ut_mesh_create: vertex 5 has more than 4 non-zero bone weights")
    bad = t.copy(); bad[7, 1] = v.shape[0]
    rc, msg = create(v, bad, w)
    assert rc == -1 and "triangle 7 names vertex 788" in msg
    bad = w.copy(); bad[3, 0] = np.nan
    rc, msg = create(v, t, bad)
    assert rc == -1 and "weight [3][0] is not finite" in msg
    bad = v.copy(); bad[9, 2] = np.inf
    rc, msg = create(bad, t, w)
    assert rc == -1 and "vertex 9" in msg
    nv = 5056 + 1
    rc, msg = create(np.zeros((nv, 3), np.float32), t, np.tile(w[:1], (nv, 1)))
    assert rc == -4 and "UT_MESH_MAX_VERTICES" in msg
    rc, msg = create(v[:0], t[:0], w[:0])
    assert rc == -1 and "no vertices" in msg
    assert lib.ut_mesh_destroy(None) == 0 and lib.ut_mesh_counts(None, None, None) == -1
