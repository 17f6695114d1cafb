"""Loop ICP (vilf_icp.hip) at its edges: one step against an exact Umeyama step on hard geometries (tests/icp_exact.py), the grown search grid and every shell of
the search, the gate at equality, empty inputs, each stopping criterion, and source sizes around the reduction tree. Every precondition is asserted on the numpy
restatement (tests/icp_reference.py) or on the exact reference before the device is looked at; the CPU tests below run those preconditions alone."""
import functools

import numpy as np
import pytest

import icp_exact as X
import icp_reference as R
from test_loop_icp import _same_bits, _store, _tolerances

F = np.float32
POSES2 = np.zeros((2, 6))


# ---- what is known before the device is looked at -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_case(name):
    return X.step_case(name)


@functools.lru_cache(maxsize=None)
def _grid_case(which):
    """(tgt, src, S, T, params, ref, cell, growths) of a search case, with its preconditions"""
    tgt, src = dict(big=X.big_scene, line=X.line_scene, point=X.point_scene)[which]()
    p = R.Params(history_keyframes=0, max_iterations=1, max_correspondence_distance=200.0)
    S, T = X.filtered(src, p), X.filtered(tgt, p)
    ref = R.align(S, T, p)
    cell, grown = X.grid_cell(T)
    d = np.sqrt(ref["first_search"][1].astype(np.float64))
    # the restatement's neighbours by brute force as well: the tree only proposes
    d2 = R.d2_float(S[:, None, :3], T[None, :, :3])
    assert np.array_equal(ref["first_search"][1], d2.min(1)) and np.array_equal(ref["first_search"][0], np.argmax(d2 == d2.min(1)[:, None], axis=1))
    if which == "big":
        assert 2500 <= len(T) <= 3600 and 750 <= len(S) <= 850, (len(T), len(S))
        assert grown >= 4, (float(cell), grown)
        buckets = [int(((d >= (r - 1) * float(cell)) & (d < r * float(cell))).sum()) for r in range(1, 7)] + [int((d >= 6 * float(cell)).sum())]
        assert min(buckets) >= 20, buckets
        lo, hi = T[:, :3].min(0), T[:, :3].max(0)
        assert ((S[:, :3] < lo) | (S[:, :3] > hi)).any(1).sum() >= 10                  # queries outside the grid's box
    elif which == "line":
        ext = (T[:, :3].max(0) - T[:, :3].min(0))
        assert grown == 0 and ext[1] == 0 and ext[2] == 0 and ext[0] / float(cell) > 100          # N x 1 x 1 cells
        assert (d > 6 * float(cell)).sum() >= 10 and (d < float(cell)).sum() >= 10
    else:
        assert len(T) == 1 and grown == 0 and (d > 6 * float(cell)).sum() >= 2 and (d == 0).sum() == 1
    return tgt, src, S, T, p, ref, cell, grown


def _generic():
    c = _step_case("generic")
    return c["tgt"], c["src"]


CRITERIA = {
    "iterations": (dict(max_iterations=2), R.ITERATIONS, 2),
    "transform": (dict(), R.TRANSFORM, None),
    "abs_mse": (dict(rotation_threshold=2.0, euclidean_fitness_epsilon=1e3), R.ABS_MSE, None),
    "rel_mse": (dict(rotation_threshold=2.0, euclidean_fitness_epsilon=0.0, mse_relative=0.5), R.REL_MSE, None),
    "copy": (dict(rotation_threshold=2.0, euclidean_fitness_epsilon=0.0, max_iterations=4), R.ITERATIONS, 4),
}


@functools.lru_cache(maxsize=None)
def _criterion_case(name):
    over, crit, rounds = CRITERIA[name]
    tgt, src = _generic()
    if name == "rel_mse":                                 # a source that no rigid motion fits: the mse settles above zero and its relative change falls below one half
        src = X.pad(X.noisy_source(tgt[:, :3]))
    if name == "copy":                                    # no coordinate is 0, so a step of 1e-16 leaves every float where it is and every d2 stays 0
        tgt = X.pad(X.lattice36((5.0, 5.0, 0.25)))
        src = tgt.copy()
    p = R.Params(history_keyframes=0, **over)
    S, T = X.filtered(src, p), X.filtered(tgt, p)
    ref = R.align_both(S, T, p)
    assert ref["criterion"] == crit and ref["converged"] and ref["stable"], (name, ref["criterion"], ref["iterations"])
    if rounds is not None:
        assert ref["iterations"] == rounds
    if name == "copy":
        # every comparison of this run is between exact zeros: |0 - 0| < 0 is false, 0 / 0 is NaN and NaN < x is false. No margin is needed, none is there.
        assert all(h["mse"] == 0.0 for h in ref["rounds"]) and [h["criterion"] for h in ref["rounds"]] == [R.NONE] * 3 + [R.ITERATIONS]
    else:
        assert ref["margin"] > 1e-3, (name, ref["margin"])
    if name == "rel_mse":
        assert ref["iterations"] >= 3 and ref["rounds"][-1]["mse"] > 1e-4
    return tgt, src, p, over, ref


@functools.lru_cache(maxsize=None)
def _gate_case(drop_one):
    tgt, src = X.gate_scene(drop_one)
    p = R.Params(history_keyframes=0, max_iterations=1, max_correspondence_distance=5.0)
    S, T = X.filtered(src, p), X.filtered(tgt, p)
    ref = R.align(S, T, p)
    idx, d2 = ref["first_search"]
    at = {tuple(S[i, :3]): (int(idx[i]), d2[i]) for i in range(len(S))}
    assert at[(3.0, 4.0, 0.0)][1] == F(25.0) and tuple(T[at[(3.0, 4.0, 0.0)][0], :3]) == (0.0, 0.0, 0.0)
    assert F(25.0) < at[(23.0, 4.0, 0.0)][1] <= F(25.0) + 4 * np.spacing(F(25.0)) and T[at[(23.0, 4.0, 0.0)][0], 0] == 20.0       # a few float spacings beyond the gate
    if drop_one:
        assert ref["n_correspondences"] == 2 and ref["criterion"] == R.NO_CORRESPONDENCES and ref["iterations"] == 0 and not ref["converged"] and not ref["accepted"]
        assert np.array_equal(ref["transform"], np.eye(4, dtype=F)) and np.isfinite(ref["fitness"]) and ref["fitness"] > 6.0
    else:
        assert ref["n_correspondences"] == 3 and ref["iterations"] == 1 and ref["criterion"] == R.ITERATIONS
    return tgt, src, p, ref


@functools.lru_cache(maxsize=None)
def _tree_case():
    clouds, pairs, over = X.tree_scene()
    p = R.Params(**over)
    T = X.filtered(clouds[0], p)
    assert len(T) == 600
    ref = []
    for (_, k), ns in zip(pairs, X.TREE_SIZES + [5, 0]):
        S = X.filtered(clouds[k], p)
        assert len(S) == ns
        ref.append(R.align_both(S, T, p))
    assert [r["rounds"][0]["n_correspondences"] for r in ref] == X.TREE_SIZES + [2, 0]
    assert [r["criterion"] for r in ref[-2:]] == [R.NO_CORRESPONDENCES] * 2 and all(r["iterations"] >= 2 for r in ref[:-2])
    keep = [i for i, r in enumerate(ref) if r["stable"] and r["margin"] > 1e-3]
    assert len(ref) - len(keep) <= 1, [(r["stable"], r["margin"]) for r in ref]
    return clouds, pairs, over, ref, keep


# ---- CPU: the references against each other, and every precondition ----------------------------------------------------------------------
@pytest.mark.parametrize("name", X.STEP_CASES)
def test_restatement_against_the_exact_step(name):
    """umeyama64 (fp64 raw sums + LAPACK), both summation orders, against exact_step: within one float32 spacing in R (at 1) and in t (at its largest entry)"""
    c = _step_case(name)
    ex = c["exact"]
    if name in X.FULL_CASES:
        assert c["dist_R"] <= X.U32 and c["dist_t"] <= float(X.ulp32(np.abs(ex["t"]).max()))
        assert np.abs(ex["R"].T @ ex["R"] - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(ex["R"]) - 1.0) < 1e-15
        assert ex["sign"] == (-1 if name.startswith("mirrored") else 1)
        assert (ex["sigma"][2] == 0.0 or ex["sigma"][2] < 1e-50) == (name in ("planar_target", "planar_both", "three")), ex["sigma"]
        assert np.array_equal(R.umeyama(c["Ss"], c["Ts"])[:3, :3], R.umeyama64(c["Ss"], c["Ts"])[0].astype(F))
    else:
        assert ex["sigma"][1] < 1e-50 * max(ex["sigma"][0], 1.0), ex["sigma"]                  # rank one (collinear) or zero (one target point)
        assert (ex["sigma"][0] > 1.0) == (name == "collinear")
        assert c["dist_t"] < 1e-13 and (name != "collinear" or c["dist_dir"] < 1e-13)
    assert c["n"] == {"three": 3, "collinear": 12, "one_target": 4}.get(name, 36)
    if name == "three":
        assert len(c["S"]) == 4 and float(c["ref"]["first_search"][1].max()) > 25.0


def test_exact_step_recovers_a_known_motion_and_the_mean_is_exact():
    rng = np.random.default_rng(2)
    S = rng.integers(-64, 64, (20, 3)).astype(F) / 4
    Rz = X.rot((0.0, 0.0, np.pi / 2)).round()                        # a quarter turn: exact in float
    T = (S.astype(np.float64) @ Rz.T + np.array([1.0, -2.0, 0.5])).astype(F)
    ex = X.exact_step(S, T)
    assert np.abs(ex["R"] - Rz).max() < 1e-15 and np.abs(ex["t"] - [1.0, -2.0, 0.5]).max() < 1e-15 and ex["sign"] == 1
    d2 = np.array([1.0, 2.0 ** -30, 2.0 ** -60], dtype=F)
    assert X.exact_mse(d2) == (1.0 + 2.0 ** -30) / 3.0 and X.mse_error_in_units(X.exact_mse(d2), d2) <= 1.0
    assert X.mse_error_in_units(0.0, np.zeros(3, dtype=F)) == 0.0 and X.mse_error_in_units(1e-300, np.zeros(3, dtype=F)) == float("inf")


def test_restatement_divides_as_ieee_does():
    """rule 4 on an exact copy: 0 / 0 is NaN and NaN is not below mse_relative, so the run ends by the iteration count (it raised ZeroDivisionError before)"""
    _, _, _, _, ref = _criterion_case("copy")
    assert ref["iterations"] == 4 and ref["criterion"] == R.ITERATIONS


@pytest.mark.parametrize("which", ["big", "line", "point"])
def test_search_scene_preconditions(which):
    _grid_case(which)


def test_gate_criteria_and_tree_preconditions():
    _gate_case(False), _gate_case(True)
    for name in CRITERIA:
        _criterion_case(name)
    _tree_case()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def _record_follows_the_header(h, M):
    """cos_angle and translation_sqr of a round's record: the header's expressions in fp64 on the float entries of the step M, to the bit"""
    m = M.astype(np.float64)
    cosa = 0.5 * (((m[0, 0] + m[1, 1]) + m[2, 2]) - 1.0)
    tsq = (m[0, 3] * m[0, 3] + m[1, 3] * m[1, 3]) + m[2, 3] * m[2, 3]
    assert h["cos_angle"] == cosa and h["translation_sqr"] == tsq, (h, cosa, tsq)


@pytest.mark.gpu
@pytest.mark.parametrize("name", X.STEP_CASES)
def test_one_step_against_the_exact_step(solver, name):
    """max_iterations = 1, identity poses, no guess: final = T_1. The first-round neighbours equal the restatement's to the bit, so the exact step is computed from the
    device's own correspondences. Tolerance per entry of T: one float32 spacing at the exact entry + 10 x the restatement's own fp64 distance from the exact value
    (largest entry of the block, both summation orders); nothing in it comes from the device. Below rank two (collinear, one target point) the rotation is not
    determined and the invariants are asserted instead. Measured distances: DESIGN.md section 3g."""
    c = _step_case(name)
    ex, ref = c["exact"], c["ref"]
    icp = _store(solver, [c["tgt"], c["src"]], history_keyframes=0, max_iterations=1, **c["over"])
    assert _same_bits(icp.submap(1, 0, 0, POSES2), c["S"]) and _same_bits(icp.submap(0, 0, 0, POSES2), c["T"])
    g = icp.align(0, 1, POSES2)
    hist = icp.history(0)
    gi, gd = icp.search(0, 0)
    assert np.array_equal(gi, ref["first_search"][0]) and _same_bits(gd, ref["first_search"][1].astype(F))
    assert (g["converged"], g["criterion"], g["iterations"], g["n_correspondences"]) == (1, R.ITERATIONS, 1, c["n"]) and len(hist) == 1
    assert (hist[0]["n_correspondences"], hist[0]["criterion"]) == (c["n"], R.ITERATIONS)
    M = g["transform"]
    assert M.dtype == F and np.isfinite(M).all() and np.array_equal(M[3], [0, 0, 0, 1])
    # the record of the round: the mse within n 2^-53 of the exact mean (any summation order over non-negative terms, one rounding per sum and one for the division)
    units = X.mse_error_in_units(hist[0]["mse"], gd[c["ok"]])
    assert units <= c["n"], (units, c["n"])
    assert g["final_mse"] == hist[0]["mse"]
    _record_follows_the_header(hist[0], M)
    if name in X.FULL_CASES:
        d = np.abs(M[:3].astype(np.float64) - np.column_stack([ex["R"], ex["t"]]))
        print(f"{name}: worst distance from the exact step: R {d[:, :3].max():.3e} ({(d[:, :3] / c['tol'][:, :3]).max():.3f} of its tolerance), "
              f"t {d[:, 3].max():.3e} ({(d[:, 3] / c['tol'][:, 3]).max():.3f}); restatement R {c['dist_R']:.2e} t {c['dist_t']:.2e}; mse {units:.2f} x 2^-53")
        assert (d <= c["tol"]).all(), (name, d / c["tol"])
    else:
        Rg, tg = M[:3, :3].astype(np.float64), M[:3, 3].astype(np.float64)
        orth, det = float(np.abs(Rg.T @ Rg - np.eye(3)).max()), float(np.linalg.det(Rg))
        res = np.abs(X.residual_of_means(Rg, tg, ex))
        tol = X.means_tolerance(c)
        line = ""
        if name == "collinear":
            # the principal direction: exact value d, one float32 spacing at its entries + R's own rounding to float (half a spacing at 1 per entry) + 10 x the restatement's
            dd = np.abs(Rg @ c["dir_s"] - c["dir_t"])
            dtol = X.ulp32(c["dir_t"]) + 0.5 * X.U32 * np.abs(c["dir_s"]).sum() + 10.0 * c["dist_dir"]
            line = f", direction {dd.max():.3e} ({(dd / dtol).max():.3f} of its tolerance)"
        print(f"{name}: |R^T R - I| {orth:.3e}, det R - 1 {det - 1.0:.3e}, |R mean_s + t - mean_t| {res.max():.3e} ({(res / tol).max():.3f} of its tolerance){line}")
        assert orth <= 4 * X.U32 and abs(det - 1.0) <= 4 * X.U32
        assert (res <= tol).all(), (res, tol)
        if name == "collinear":
            assert (dd <= dtol).all(), (dd, dtol)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["big", "line", "point"])
def test_search_on_a_grown_grid_and_in_every_shell(solver, which):
    """big: 1000 m x 1000 m x 40 m, so the 1.6 m cell grows (six times: 6.1 m) and the float cell size enters the shell cut-off; at least 20 queries have their
    nearest point in each of the shells 1 .. 6 and beyond the last (the whole-target scan), counted on the restatement. line: N x 1 x 1 cells. point: one cell."""
    tgt, src, S, T, p, ref, cell, grown = _grid_case(which)
    icp = _store(solver, [tgt, src], history_keyframes=0, max_iterations=1, max_correspondence_distance=200.0)
    assert _same_bits(icp.submap(1, 0, 0, POSES2), S) and _same_bits(icp.submap(0, 0, 0, POSES2), T)
    g = icp.align(0, 1, POSES2)
    assert (g["n_source"], g["n_target"], g["iterations"]) == (len(S), len(T), ref["iterations"])
    fitness_search = ref["fitness_search"]
    if which != "big":
        # a target on a line or of one point leaves the step's rotation open (rank one or zero), so the restatement's moved source is not the device's. The fitness
        # pass is compared with the restatement's search (checked by brute force) over the source moved by the device's own step, in the header's float arithmetic.
        moved = R.transform(g["transform"][:3], S)
        fitness_search = R.Target(T).nearest(moved)
        d2 = R.d2_float(moved[:, None, :3], T[None, :, :3])
        assert np.array_equal(fitness_search[1], d2.min(1)) and np.array_equal(fitness_search[0], np.argmax(d2 == d2.min(1)[:, None], axis=1))
    for w, (ri, rd) in ((0, ref["first_search"]), (1, fitness_search)):
        gi, gd = icp.search(0, w)
        bad = np.flatnonzero(gi != ri)
        assert len(bad) == 0, (which, w, len(bad), bad[:10], gd[bad[:10]], rd[bad[:10]])
        assert _same_bits(gd, rd.astype(F)), (which, w)


@pytest.mark.gpu
def test_gate_at_equality_and_two_correspondences(solver):
    for drop_one in (False, True):
        tgt, src, p, ref = _gate_case(drop_one)
        icp = _store(solver, [tgt, src], history_keyframes=0, max_iterations=1, max_correspondence_distance=5.0)
        g = icp.align(0, 1, POSES2)
        hist = icp.history(0)
        gi, gd = icp.search(0, 0)
        assert np.array_equal(gi, ref["first_search"][0]) and _same_bits(gd, ref["first_search"][1].astype(F))
        assert len(hist) == 1 and hist[0]["n_correspondences"] == g["n_correspondences"] == (2 if drop_one else 3)
        assert (g["converged"], g["accepted"], g["criterion"], g["iterations"]) == (int(ref["converged"]), int(ref["accepted"]), ref["criterion"], ref["iterations"])
        if drop_one:
            assert g["criterion"] == R.NO_CORRESPONDENCES and g["iterations"] == 0 and not g["converged"]
            assert np.array_equal(g["transform"], np.eye(4, dtype=F))                    # the guess
            assert np.isfinite(g["fitness"]) and g["fitness"] == ref["fitness"] and g["fitness"] > 6.0          # no range limit: the rejected pair counts
        else:
            assert g["iterations"] == 1 and np.isfinite(g["transform"]).all()


@pytest.mark.gpu
def test_empty_source_and_empty_target(solver):
    tgt, src = _generic()
    clouds = [tgt, src, np.zeros((0, 4), dtype=F)]
    poses = np.zeros((3, 6))
    p = R.Params(history_keyframes=0)
    icp = _store(solver, clouds, history_keyframes=0)
    first = icp.align(0, 1, poses)
    first_hist = icp.history(0)
    assert first["converged"] and first["iterations"] >= 2
    for prev, curr in [(0, 2), (2, 1), (2, 2)]:                      # empty source, empty target, both
        ref = R.align(clouds[curr], clouds[prev], p)
        assert ref["fitness"] == R.DBL_MAX and ref["criterion"] == R.NO_CORRESPONDENCES and not ref["accepted"] and ref["n_correspondences"] == 0
        g = icp.align(prev, curr, poses)
        assert g["fitness"] == R.DBL_MAX and not g["accepted"] and not g["converged"] and g["criterion"] == R.NO_CORRESPONDENCES and g["iterations"] == 0
        assert (g["n_source"], g["n_target"], g["n_correspondences"]) == (ref["n_source"], ref["n_target"], 0) == (len(clouds[curr]), len(clouds[prev]), 0)
        assert np.array_equal(g["transform"], np.eye(4, dtype=F))
        hist = icp.history(0)
        assert len(hist) == 1 and (hist[0]["n_correspondences"], hist[0]["criterion"]) == (0, R.NO_CORRESPONDENCES)
        gi, gd = icp.search(0, 0)
        assert len(gi) == len(clouds[curr]) and (gi == -1).all() and np.isinf(gd).all()
    again = icp.align(0, 1, poses)                                   # the store is as it was
    for k, v in first.items():
        assert _same_bits(np.asarray(v), np.asarray(again[k])), k
    assert icp.history(0) == first_hist


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CRITERIA))
def test_each_stopping_criterion_is_reached(solver, name):
    tgt, src, p, over, ref = _criterion_case(name)
    icp = _store(solver, [tgt, src], history_keyframes=0, **over)
    g = icp.align(0, 1, POSES2)
    hist = icp.history(0)
    print(f"{name}: criterion {g['criterion']} after {g['iterations']} rounds, mse " + " ".join(f"{h['mse']:.3e}" for h in hist))
    assert (g["converged"], g["criterion"], g["iterations"]) == (1, ref["criterion"], ref["iterations"])
    assert [h["criterion"] for h in hist] == [h["criterion"] for h in ref["rounds"]]
    assert [h["n_correspondences"] for h in hist] == [h["n_correspondences"] for h in ref["rounds"]]
    if name == "copy":
        assert all(h["mse"] == 0.0 for h in hist) and len(hist) == 4


@pytest.mark.gpu
def test_source_sizes_around_the_reduction_tree_in_one_batch(solver):
    """a wave of 64, 4 waves per block of 256, blocks in order: 3 .. 513 source points, with a pair of 2 correspondences and an empty source in the same batch"""
    clouds, pairs, over, ref, keep = _tree_case()
    poses = np.zeros((len(clouds), 6))
    icp = _store(solver, clouds, **over)
    batch = icp.align_pairs(pairs, poses)
    hist = [icp.history(i) for i in range(len(pairs))]
    for i, (a, b) in enumerate(pairs):
        one = icp.align(a, b, poses)
        for k, v in batch[i].items():
            assert _same_bits(np.asarray(v), np.asarray(one[k])), (pairs[i], k)
        assert icp.history(0) == hist[i], pairs[i]
    for i in keep:
        g, r = batch[i], ref[i]
        assert (g["converged"], g["criterion"], g["iterations"]) == (int(r["converged"]), r["criterion"], r["iterations"]), (pairs[i], g)
        assert (g["n_source"], g["n_target"]) == (r["n_source"], r["n_target"])
        assert [h["n_correspondences"] for h in hist[i]] == [h["n_correspondences"] for h in r["rounds"]]
        if r["n_source"] == 0:
            assert g["fitness"] == R.DBL_MAX
            continue
        tol, _ = _tolerances(r, [clouds[pairs[i][0]], clouds[pairs[i][1]]])
        d = dict(translation=float(np.abs(g["transform"][:3, 3].astype(np.float64) - r["transform"][:3, 3]).max()),
                 angle=abs(R.rotation_angle(g["transform"]) - R.rotation_angle(r["transform"])), fitness=abs(g["fitness"] - r["fitness"]),
                 mse=max(abs(x["mse"] - y["mse"]) for x, y in zip(hist[i], r["rounds"])))
        print(f"ns {r['n_source']}: iterations {g['iterations']} criterion {g['criterion']}; differences " + ", ".join(f"{k} {v:.3e} (tol {tol[k]:.3e})" for k, v in d.items()))
        for k in d:
            assert d[k] <= tol[k], (pairs[i], k, d[k], tol[k])
