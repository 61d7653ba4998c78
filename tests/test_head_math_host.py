"""Host tests of csrc/ut_math.h, the float64 math of the head's decode (Procrustes rotation, 4x4 inverse and product): the
header compiles with the host C++ compiler as it stands, so the same routines the device runs are compared here with numpy's
float64 LAPACK on inputs the product's one synthetic network never emits.

Tolerances are not taken from the routine under test: every reference is computed twice in float64 by different routes (SVD of H
and of H^T; inverse of A and of A^T), and the routine is allowed 16 x the distance between the two, with a floor of 64 ulp."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import head_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "absolutetrack_amd", "csrc")
FLOOR = 64 * hc.ULP64
MARGIN = 16.0

WRAPPER = r"""
#include "ut_math.h"
extern "C" {
void kabsch_n(const double* h, double* r, int n) {
  for (int s = 0; s < n; ++s) {
    double hh[3][3], rr[3][3];
    for (int i = 0; i < 9; ++i) hh[i / 3][i % 3] = h[9 * s + i];
    ut::kabsch_rotation(hh, rr);
    for (int i = 0; i < 9; ++i) r[9 * s + i] = rr[i / 3][i % 3];
  }
}
void inv4_n(const double* a, double* out, int* ok, int n) {
  for (int s = 0; s < n; ++s) ok[s] = ut::inv4(a + 16 * s, out + 16 * s) ? 1 : 0;
}
void mul4_n(const double* a, const double* b, double* c, int n) {
  for (int s = 0; s < n; ++s) ut::mul4(a + 16 * s, b + 16 * s, c + 16 * s);
}
}
"""


def build_wrapper(out_dir, include_dir=CSRC):
    """ut_math.h of `include_dir` behind a C ABI, as a ctypes library (None without a host C++ compiler)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        return None
    src, lib = os.path.join(str(out_dir), "ut_math_host.cpp"), os.path.join(str(out_dir), "libut_math_host.so")
    with open(src, "w") as fh:
        fh.write(WRAPPER)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", include_dir, src, "-o", lib])
    return ctypes.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def kabsch(lib, h):
    h = np.ascontiguousarray(h, np.float64)
    r = np.zeros_like(h)
    lib.kabsch_n(_p(h), _p(r), h.shape[0])
    return r


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = build_wrapper(tmp_path_factory.mktemp("ut_math_host"))
    if out is None:
        pytest.skip("needs a host C++ compiler")
    return out


FAMILIES = ["random"] + list(hc.WELL_POSED)
N_PER_FAMILY = 400


def well_posed_cases():
    """[(family, H [n,3,3])], the same on every call."""
    rng = np.random.default_rng(2024)
    return [(name, hc.cross_covariance(hc.targets(name, rng, N_PER_FAMILY))) for name in FAMILIES]


@pytest.mark.parametrize("family", FAMILIES)
def test_kabsch_rotation_against_numpy_svd(lib, family):
    """kabsch_rotation against V diag(1, 1, det(V U^T)) U^T from numpy.linalg.svd, on cross-covariances of the real source points
    (fp32-rounded) and 400 targets per family: random over six decades of magnitude; rigid images; anisotropically scaled
    (1.3, 1.0, 0.6); the same mirrored on each axis in turn; third factor +-1e-7; exactly coplanar.  Every case is compared, each
    within max(16 x |R_svd(H) - R_svd(H^T)|, 64 ulp) of its own reference pair.  The generator is asserted to be well posed where
    the answer depends on it: wherever the reflection rule fires or the third singular value is below 1e-3 of the first, the
    answer hangs on the third singular pair, and (s2 - s3) / s1 must exceed 1e-3; every scaled family also keeps (s1 - s2) / s1
    above 1e-3.  (A rigid image has s2 = s3 by the source's symmetry, legitimately: its answer is the polar factor of a
    well-conditioned H and depends on no single vector.)
    Measured (x86-64, g++ -O2), max |R - R_ref| (largest allowance used) per family: random 1.3e-14 (2.3e-13); rigid 3.1e-15
    (5.0e-14); aniso 6.5e-15 (1.0e-13); mirror_x 1.7e-14 (2.9e-13), mirror_y 1.6e-14 (2.5e-13), mirror_z 1.8e-14 (3.0e-13);
    third_+1e-7 8.2e-15 (1.3e-13), third_-1e-7 8.5e-15 (1.4e-13); coplanar 1.7e-15 (2.8e-14); the worst case uses 0.16 of its
    own allowance.  Reflections: 197 of 400 random cases, every mirrored and third_-1e-7 case, 214 coplanar ones (s3 = 0: the
    SVD's choice), no other; smallest needed (s2 - s3) / s1 2.5e-2.  These families give the same bits with the header as it
    was before the rank test was added."""
    h = dict(well_posed_cases())[family]
    ra, rb, s = hc.reference_rotation(h)
    reflected = np.linalg.det(np.swapaxes(np.linalg.svd(h)[2], -1, -2) @ np.swapaxes(np.linalg.svd(h)[0], -1, -2)) < 0
    gap23, gap12 = (s[:, 1] - s[:, 2]) / s[:, 0], (s[:, 0] - s[:, 1]) / s[:, 0]
    needs23 = reflected | (s[:, 2] < 1e-3 * s[:, 0])
    assert (gap23[needs23] > 1e-3).all(), (family, gap23[needs23].min())
    assert (s[:, 1] > 1e-3 * s[:, 0]).all()
    if family not in ("random", "rigid"):
        assert (gap12 > 1e-3).all(), (family, gap12.min())
    if family.startswith("mirror") or family == "third_-1e-7":
        assert reflected.all()
    elif family == "random":
        assert 100 < reflected.sum() < 300
    elif family != "coplanar":          # s3 = 0: the sign of det(V U^T) is the SVD's choice, and R does not depend on it
        assert not reflected.any()
    got = kabsch(lib, h)
    err = np.abs(got - ra).max(axis=(1, 2))
    allow = np.maximum(MARGIN * np.abs(ra - rb).max(axis=(1, 2)), FLOOR)
    print(f"\nkabsch {family}: max err {err.max():.2e}, largest allowance {allow.max():.2e}, worst err/allow "
          f"{(err / allow).max():.2f}, reflections {int(reflected.sum())}, min gap23 (needed) "
          f"{gap23[needs23].min() if needs23.any() else float('nan'):.2e}")
    assert (err <= allow).all(), (family, int(np.argmax(err / allow)), err.max())
    orth, det = hc.rotation_defects(got)
    assert orth < 1e-12 and det < 1e-12


@pytest.mark.parametrize("family", hc.RANK_LE_1)
def test_kabsch_rotation_is_a_rotation_at_rank_one_and_zero(lib, family):
    """Cross-covariances of rank <= 1 - collinear targets, seven coincident targets, all-zero targets - have no unique answer
    (but H = 0: the reference's svd(0) is U = V = I, so R = I), so properties are asserted: |R R^T - I| < 1e-12, det R = +1 to
    1e-12, R u1 = v1 for the leading singular pair where there is one, and R == I exactly for H = 0.  Before the relative rank
    test in kabsch_rotation: |R R^T - I| = 0.997 (collinear), 1.0 (coincident), R = 0 for H = 0.  Now: 1.3e-15, 4.4e-16, 0;
    |det R - 1| 1.6e-15, |R u1 - v1| 8.9e-16."""
    h = hc.cross_covariance(hc.targets(family, np.random.default_rng(7), 300))
    got = kabsch(lib, h)
    if family == "zero":
        assert not h.any()
        assert (got == np.eye(3)[None]).all()
        return
    orth, det = hc.rotation_defects(got)
    lead = 0.0
    if family == "collinear":
        u, s, vt = np.linalg.svd(h)
        assert (s[:, 1] < 1e-12 * s[:, 0]).all()
        lead = np.abs(np.einsum("nij,nj->ni", got, u[:, :, 0]) - vt[:, 0, :]).max()
    print(f"\nkabsch {family}: |R R^T - I| {orth:.2e}, |det - 1| {det:.2e}, |R u1 - v1| {lead:.2e}")
    assert orth < 1e-12 and det < 1e-12 and lead < 1e-12


def _inverse_cases():
    rng = np.random.default_rng(11)
    n = 400
    rigid = hc.rigid4(rng, n)
    f = np.tile(np.eye(4), (n, 1, 1))
    f[:, 2, 2] = rng.uniform(50.0, 400.0, n) / 200.0          # the FTL's S = diag(1, 1, f / 200, 1)
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0])
    return {"rigid": rigid, "scaled_rigid": rigid @ f, "canonical": np.linalg.inv(f) @ rigid @ hc.rigid4(rng, n) @ f,
            "mirrored": mirror[None] @ rigid, "rigid_fp32": rigid.astype(np.float32).astype(np.float64)}


@pytest.mark.parametrize("family", ["rigid", "scaled_rigid", "canonical", "mirrored", "rigid_fp32"])
def test_inv4_mul4_against_numpy(lib, family):
    """inv4 against numpy.linalg.inv and mul4 against the float64 matrix product on the 4x4s the head inverts and multiplies:
    rigid transforms (rotations to pi, translations to 2 m), X S and S0^-1 X0 Xv S (FTL, f / 200 in 0.25 .. 2), mirrored ones
    (right hands), fp32-rounded ones (not exactly orthogonal, as the kernels load them).  Allowed: 16 x the distance between
    inv(A) and inv(A^T)^T (for the product: between the float64 and the long double product), floor 64 ulp, relative to the
    result's largest entry.  Measured: inv4 at most 7.7e-16 relative (allowance: the 1.42e-14 floor everywhere), mul4 4.4e-16,
    |inv4(A) A - I| at most 1.8e-15."""
    a = np.ascontiguousarray(_inverse_cases()[family])
    n = a.shape[0]
    got = np.zeros_like(a)
    ok = np.zeros(n, np.int32)
    lib.inv4_n(_p(a), _p(got), _p(ok), n)
    assert ok.all()
    ra, rb = np.linalg.inv(a), np.swapaxes(np.linalg.inv(np.swapaxes(a, 1, 2)), 1, 2)
    scale = np.abs(ra).max(axis=(1, 2))
    err = np.abs(got - ra).max(axis=(1, 2)) / scale
    allow = np.maximum(MARGIN * np.abs(ra - rb).max(axis=(1, 2)) / scale, FLOOR)
    assert (err <= allow).all(), (family, err.max())
    b = np.ascontiguousarray(np.roll(a, 1, axis=0))
    prod = np.zeros_like(a)
    lib.mul4_n(_p(a), _p(b), _p(prod), n)
    pa = a @ b
    pb = (a.astype(np.longdouble) @ b.astype(np.longdouble)).astype(np.float64)
    pscale = np.abs(pa).max(axis=(1, 2))
    perr = np.abs(prod - pa).max(axis=(1, 2)) / pscale
    pallow = np.maximum(MARGIN * np.abs(pa - pb).max(axis=(1, 2)) / pscale, FLOOR)
    ident = np.zeros_like(a)
    lib.mul4_n(_p(got), _p(a), _p(ident), n)
    resid = np.abs(ident - np.eye(4)).max()
    print(f"\ninv4 {family}: {err.max():.2e} (allow {allow.min():.2e} .. {allow.max():.2e}); mul4 {perr.max():.2e}; "
          f"|inv4(A) A - I| {resid:.2e}")
    assert (perr <= pallow).all(), (family, perr.max())
    assert resid < 1e-12
