"""CPU tests of tests/step_cases.py, the yardstick of tests/test_gpu_fit_step.py: the float64 restatements' Jacobians on the
blended skinning tables against central differences, the float32 restatement against the float64 one after one step on
every case the GPU test runs (equal decisions; the distances the GPU bounds come from), the evidence that one step sees a
wrong linearisation, and the searched and constructed cases (rejected first trials, hidden fingers, steps into the wall)."""
import numpy as np
import pytest

import fit_cases as fc
import mesh_cases as mc
import scale_cases as sc
import step_cases as st


def _central(hm, ang, m, centroid, scale=None, h=1e-5):
    """Worst |analytic - central difference| of a column over the column's largest entry, fc.jacobian (scale None) or
    sc.jacobian; columns nobody moves must be exactly zero."""
    b = len(ang)
    if scale is None:
        jac, n_par = fc.jacobian(hm, ang, m, centroid), 26
        at = lambda d: fc.forward(hm, *fc.apply_step(ang, m, centroid, d))                                # noqa: E731
    else:
        jac, n_par = sc.jacobian(hm, scale, ang, m, centroid), 27

        def at(d):
            a, mm, s = sc.apply_step(ang, m, scale, centroid, d)
            return sc.forward(hm, s, a, mm)
    worst = 0.0
    for k in range(n_par):
        d = np.zeros((b, n_par))
        d[:, k] = h
        fd = ((at(d) - at(-d)) / (2 * h)).reshape(b, 63)
        size = np.abs(fd).max(1)
        moving = size > 0
        assert moving.any(), k
        worst = max(worst, float((np.abs(jac[:, :, k] - fd).max(1)[moving] / size[moving]).max()))
        assert np.array_equal(jac[~moving, :, k], np.zeros_like(jac[~moving, :, k]))
    return worst


@pytest.mark.parametrize("table", ["a", "b", "mixed"])
def test_jacobians_match_central_differences_on_blended_tables(table):
    """fc.jacobian and sc.jacobian (scale 0.9 / 1.1) on the 24 label poses and on their starts, both hands, to the bound of
    test_fit_host.test_jacobian_matches_central_differences: 1e-6 of a column's largest entry.  No angle of these poses
    lies inside so3_exp_map's clamp (|angle| < 0.01 rad), where the analytic Jacobian deliberately differs.

    A run on TABLE_A with poses chosen without regard to the clamp had given 8.8e-6.  The clamp explains it: the same
    measurement on the 24 label poses closest to it (smallest |angle| 1e-5 .. 3e-3 rad) is printed below and is of that
    size on the stock table as well, where 20 landmarks do not blend at all; away from the clamp the blended tables are as
    close as the stock one.  The restatement is right on blends."""
    p = st.poses()
    hm = st.skeleton(table)
    m = fc.effective_wrist(p["xf"], p["hand"], 1.0, np.float64)
    m0 = fc.effective_wrist(p["xf0"].astype(np.float64), p["hand"], 1.0, np.float64)
    centroid = st.label_targets(hm, p["ja"], p["xf"], p["hand"]).astype(np.float64).mean(1)
    assert set(p["hand"]) == {0, 1}
    assert min(np.abs(p["ja"][:, :20]).min(), np.abs(p["ja0"][:, :20]).min()) >= st.CLAMP
    s = np.where(np.arange(st.N) % 4 < 2, 0.9, 1.1)
    for what, ang, wrist in (("labels", p["ja"][:, :20].copy(), m), ("starts", p["ja0"][:, :20].astype(np.float64), m0)):
        plain, scaled = _central(hm, ang, wrist, centroid), _central(hm, ang, wrist, centroid, s)
        print(f"table {table}, {what}: fc.jacobian {plain:.3e}, sc.jacobian {scaled:.3e} of a column's largest entry")
        assert plain <= 1e-6 and scaled <= 1e-6


def test_the_clamp_explains_the_larger_differences():
    """The measurement behind the docstring above: the 24 label poses with the smallest |angle|, stock table and TABLE_A.
    Inside the clamp so3_exp_map is not a rotation by the angle, the analytic Jacobian (the restatement's and the kernel's)
    ignores that on purpose, and central differences see it - on both tables alike."""
    ja, xf, hand = st.labels()
    near = np.argsort(np.abs(ja[:, :20]).min(1))[:24]
    assert np.abs(ja[near, :20]).min(1).max() < st.CLAMP
    m = fc.effective_wrist(xf[near], hand[near], 1.0, np.float64)
    got = {}
    for table in ("stock", "a"):
        hm = st.skeleton(table)
        centroid = st.label_targets(hm, ja[near], xf[near], hand[near]).astype(np.float64).mean(1)
        got[table] = _central(hm, ja[near, :20].copy(), m, centroid)
    print(f"label poses inside the clamp: central differences differ by {got['stock']:.3e} (stock), {got['a']:.3e} (TABLE_A)")
    assert got["stock"] > 1e-6 and got["a"] > 1e-6              # the clamp alone does it, with or without blends
    assert got["a"] <= 10 * got["stock"]


def test_tables_exercise_what_they_claim():
    a, b = (mc.dense_landmark_weights(st.skeleton(t)) for t in ("a", "b"))
    assert a[2, 10] == np.float32(0.375) and a[2, 9] == np.float32(0.625)          # the first entry is dead
    assert a[1, 7] == np.float32(0.75) and a[4, 16] == 1 and a[4, 0] == 0 and a[4, 2] == 0
    assert b[1, 7] == np.float32(0.75)                                            # a later zero entry kills nothing
    assert b[6, 2] == np.float32(0.5) and b[16, 12] == 1 and (b[10, 2:] == 0).all()
    mixed = st.skeleton("mixed")
    assert mixed["landmark_rest_bone_weights"].shape == (st.N, 21, 3)
    for i, t in enumerate(("a", "b", "stock")):
        assert np.array_equal(mixed["landmark_rest_bone_indices"][i], st.skeleton(t)["landmark_rest_bone_indices"])
    with pytest.raises(AssertionError):                                            # a table that does not sum to 1 is refused
        st.blend({0: ((0.5, 0.3, 0.3), (4, 3, 2))})
    with pytest.raises(AssertionError):                                            # 0.7 is dead, but so is the sum
        st.blend({2: ((0.7, 0.3, 0.375), (10, 9, 10))})


@pytest.mark.parametrize("entry", st.ENTRIES)
def test_float32_restatement_after_one_step(entry):
    """Every case of the GPU test's one-step comparison: the float32 restatements (LU and Cholesky solve) decide as the
    float64 one (first trial accepted or not, iterations, status), and lie this far from it at the worst.  Unit weights
    stay within a quarter of the project's bounds, so the GPU is held to those bounds there; the other groups' bounds are
    4 x the distances printed here."""
    for e, table, group in st.all_cases():
        if e != entry:
            continue
        r64, t64 = st.step(e, table, group, np.float64)
        for how in st.SOLVERS:
            for a, b in zip(st.decisions(r64, t64), st.decisions(*st.step(e, table, group, np.float32, 1, how))):
                assert np.array_equal(a, b), (e, table, group, how)
        assert np.all(r64["info"][:, 2] == 1) and np.all(r64["info"][:, 3] == fc.AT_MAX_ITERS) and t64[0]["accept"].all()
        d, tol = st.float32_distance(e, table, group), st.tolerance(e, table, group)
        print(f"{e:11s} {table:5s} {group:6s} float32 vs float64: angles {d['ang']:.2e} rad, landmarks {d['kp']:.2e} mm, scale "
              f"{d['scale']:.2e}, scale information {d['scale_info']:.2e} | GPU bounds {tol['ang']:.2e} rad, {tol['kp']:.2e} mm, "
              f"{tol['scale']:.2e}, {tol['scale_info']:.2e}")
        if group in ("unit", "metres"):
            assert d["ang"] <= st.ANGLE_TOL_RAD / 4 and d["kp"] <= st.KP_TOL_MM / 4 and d["scale"] <= st.SCALE_TOL / 4
            assert tol["ang"] == st.ANGLE_TOL_RAD and tol["kp"] == st.KP_TOL_MM
        step_size = fc.angle_distance(r64["ja"][:, :20], st.case(e, table, group)["init"][0][:, :20]).max()
        assert step_size > 0.05                       # a step worth comparing, not a start that is already there
        if e == "scale_free":
            assert np.abs(r64["scale"] - st.case(e, table, group)["init_scale"]).min() > 1e-3


SENSITIVITY = [("stock_table", "fit", ("a", "b", "mixed"), "unit"), ("first_wins", "fit", ("a", "b", "mixed"), "unit"),
               ("no_mirror", "fit", st.TABLES, "unit"), ("no_sigma", "scale_free", st.TABLES, "unit"),
               ("transposed", "info", st.TABLES, "aniso")]


@pytest.mark.parametrize("defect,entry,tables,group", SENSITIVITY)
def test_one_step_sees_a_wrong_linearisation(defect, entry, tables, group):
    """The float64 restatement with one defect in its linearisation (step_cases.wrong) moves the one-step result by more
    than 100 x the bound the GPU test uses for that case - in angles and in landmarks - so a kernel with that defect fails
    test_gpu_fit_step.test_one_step.  Without the mirror's sign only right hands move: left ones keep their bits."""
    for table in tables:
        c = st.case(entry, table, group)
        good, tol = st.step(entry, table, group, np.float64)[0], st.tolerance(entry, table, group)
        with st.wrong(defect):
            bad = st.restate(c, np.float64, 1)
        d = st.distance(c, bad, good)
        print(f"{defect} on {entry} {table} {group}: moves one step by {d['ang']:.3e} rad ({d['ang'] / tol['ang']:.0f} x the bound), "
              f"{d['kp']:.3e} mm ({d['kp'] / tol['kp']:.0f} x), scale {d['scale']:.3e} ({d['scale'] / tol['scale']:.0f} x)")
        assert d["ang"] > 100 * tol["ang"] and d["kp"] > 100 * tol["kp"]
        if defect == "no_sigma":
            assert d["scale"] > 100 * tol["scale"]
        if defect == "no_mirror":
            left = c["mirror"] == 0
            assert np.array_equal(bad["ja"][left], good["ja"][left]) and np.array_equal(bad["xf"][left], good["xf"][left])
    again = st.restate(st.case(entry, tables[0], group), np.float64, 1)                # the defect is gone afterwards
    assert np.array_equal(again["ja"], st.step(entry, tables[0], group, np.float64)[0]["ja"])


@pytest.mark.parametrize("entry", ["fit", "scale_free"])
def test_rejected_start_search(entry):
    """At least 8 starts whose first trial both restatements reject by 5 % or more and whose second both accept."""
    c = st.rejected_case(entry)
    n = len(c["targets"])
    print(f"{entry}: {n} rejected starts (seed, pose) {c['found']}; first trial / start cost >= {c['ratios'][:, :, 0].min():.3f}, "
          f"second <= {c['ratios'][:, :, 1].max():.3f}")
    assert 8 <= n <= st.REJECT_MAX and len(c["found"]) == n
    assert c["ratios"][:, :, 0].min() >= st.REJECT_MARGIN and c["ratios"][:, :, 1].max() <= st.ACCEPT_MARGIN
    for dt, how in st.RUNS:
        trace = []
        one = st.restate(c, dt, 1, trace, how)
        assert not trace[0]["accept"].any() and np.all(one["info"][:, 3] == fc.AT_MAX_ITERS)
        assert np.array_equal(one["ja"], c["init"][0].astype(dt)) and np.array_equal(one["xf"], c["init"][1].astype(dt))
        trace = []
        two = st.restate(c, dt, 2, trace, how)
        assert trace[1]["accept"].all() and np.allclose(trace[1]["lam"], 1e-2) and np.all(two["info"][:, 2] == 2)
    d = st.float32_distance_of(c, st.restate(c, np.float64, 2), 2)
    print(f"{entry}: second step, float32 vs float64: {d['ang']:.2e} rad, {d['kp']:.2e} mm, scale {d['scale']:.2e}")


def test_hidden_fingers_and_the_tie():
    """hidden_case: on the stock table every joint of the hidden finger is unobservable and nothing else is; on TABLE_A
    hiding landmark 3, which ties ring and middle, freezes the ring's distal joint alone.  The float64 restatement converges
    on the kept landmarks and keeps the unobservable angles."""
    for table in ("stock", "a"):
        c = st.hidden_case(table)
        if table == "stock":
            for i in range(st.N):
                f = i % 5
                assert not c["seen"][i, 4 * f:4 * f + 4].any() and c["seen"][i].sum() == 16
                assert (c["weights"][i] == 0).sum() == (4 if f in (1, 2) else 3)
        else:
            assert np.array_equal(np.nonzero(~c["seen"][0])[0], [15]) and (c["seen"] == c["seen"][0]).all()
        for dt, bound in ((np.float64, 1e-5), (np.float32, st.KP_TOL_MM)):
            r = st.restate(c, dt, 32)
            err = np.linalg.norm(st.landmarks(c, r) - c["targets"], axis=-1)[c["weights"] > 0].max()
            print(f"hidden, table {table}, {np.dtype(dt).name}: kept landmarks {err:.3e} mm, iterations max {int(r['info'][:, 2].max())}")
            assert np.all(r["info"][:, 3] == fc.CONVERGED) and err <= bound
            assert np.array_equal(r["ja"][:, :20][~c["seen"]], c["init"][0][:, :20].astype(dt)[~c["seen"]])
            assert np.all(r["ja"][:, :20][c["seen"]] != c["init"][0][:, :20].astype(dt)[c["seen"]])


def test_wall_case():
    c = st.wall_case()
    r = st.restate(c, np.float64, 1)
    print(f"into the wall: {int(c['wall'].sum())} joints of {int(c['wall'].any(1).sum())} poses")
    assert c["wall"].sum() >= 12 and c["wall"].any(1).sum() >= 8
    assert np.array_equal(r["ja"][:, :20][c["wall"]], c["bound"][c["wall"]].astype(np.float64))
    assert np.array_equal(c["init"][0][:, :20][c["wall"]], c["bound"][c["wall"]])
    lo, hi = c["limits"][..., 0], c["limits"][..., 1]
    assert np.all(r["ja"][:, :20] >= lo) and np.all(r["ja"][:, :20] <= hi)
    assert np.all((c["bound"][c["wall"]] == lo[c["wall"]]) | (c["bound"][c["wall"]] == hi[c["wall"]]))
    assert np.abs(c["bound"][c["wall"]]).min() >= st.CLAMP


def test_iteration_margins():
    """The margin of test_gpu_fit_step.test_iterations: the float32 and float64 restatements' full fits on the blended
    tables converge everywhere, and their iteration counts differ per pose by what is printed here."""
    for entry, table, group in st.ITERATION_CASES:
        it32, it64, margin, both = st.iteration_yardstick(entry, table, group)
        print(f"{entry} {table} {group}: iterations float32 LU sum {both[0].sum()} max {both[0].max()}, Cholesky sum {both[1].sum()} max "
              f"{both[1].max()}, float64 sum {it64.sum()} max {it64.max()}; the float32 runs up to {np.abs(both[0] - both[1]).max()} "
              f"apart, up to {np.abs(both - it64).max()} from float64: margin {margin}")
        assert margin >= 2 and it32.max() + margin < 32
