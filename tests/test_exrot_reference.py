"""The camera-IMU rotation calibration without a GPU: the numpy restatement of the contract text (tests/exrot_reference.py) against numpy's SVD and against the
ground truth of the synthetic cases, the arc tangent of the text against np.arctan2, FeatureManager.get_corresponding, the ctypes layouts, and the gate of
SlidingWindowEstimator (estimate_extrinsic = 2 holds the initialisation back until the calibration succeeds) with the restatement as the back-end.

The tolerances are the restatement's own differences measured on exactly these cases (seeds 0 .. 3, K = 64, 12 pushes), times a margin of 10 for other seeds;
DESIGN.md §3r quotes the same measurements. Every test prints what it measured before it asserts."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import exrot_cases as ec
import exrot_reference as er
from vil_fusion_amd import abi, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS, N_PUSH, K = (0, 1, 2, 3), 12, 64
MARGIN = 10.0
SIGMA_MEASURED = 7.1e-12        # max |sigma_k - numpy's singular value|: sigma is sqrt of an eigenvalue of A^T A, so the smallest (about 1e-6) carries eps / sigma
X_MEASURED = 5.6e-16            # max |x - numpy's last right singular vector|, up to sign
RIC_MEASURED_DEG = 7.9e-4       # the angle between the recovered ric and the ground truth after min_frames pushes (float32 points: 6e-8 relative)
RC_MEASURED_DEG = 9.5e-4        # the angle between Rc and the true relative rotation, every push


@pytest.fixture(scope="module")
def runs():
    """per seed: the pushes, the row of every push, the calibrator after the last one and after min_frames pushes its ric"""
    out = {}
    for seed in SEEDS:
        cal = er.Calibrator(n_hypotheses=K, seed=seed)
        pushes = ec.make_pushes(seed, N_PUSH)
        rows, ric10 = [], None
        for pr in pushes:
            rows.append(cal.push(pr["a"], pr["b"], pr["dq"]))
            if cal.frame_count == cal.P["min_frames"]:
                ric10 = cal.ric.copy()
        out[seed] = dict(pushes=pushes, rows=rows, cal=cal, ric10=ric10)
    return out


def test_system_agrees_with_numpy_svd(runs):
    worst_s = worst_x = 0.0
    for seed in SEEDS:
        cal, row = runs[seed]["cal"], runs[seed]["rows"][-1]
        _, _, B, _ = cal.system()
        A = B.reshape(-1, 4)                                  # the 4n x 4 matrix of the blocks, built explicitly
        assert A.shape == (4 * N_PUSH, 4)
        _, S, Vt = np.linalg.svd(A)
        worst_s = max(worst_s, np.abs(S - row["sigma"]).max())
        worst_x = max(worst_x, min(np.abs(Vt[3] - row["x"]).max(), np.abs(Vt[3] + row["x"]).max()))
    print(f"max |sigma - svd| {worst_s:.3e}, max |x -+ svd| {worst_x:.3e}")
    assert worst_s <= MARGIN * SIGMA_MEASURED and worst_x <= MARGIN * X_MEASURED


def test_recovers_the_ground_truth_ric_at_min_frames(runs):
    worst = 0.0
    for seed in SEEDS:
        rows = runs[seed]["rows"]
        assert [r["ok"] for r in rows[:9]] == [False] * 9 and rows[9]["ok"], "the first success is push min_frames"
        assert rows[9]["sigma"][2] > 0.25
        worst = max(worst, ec.angle_between(runs[seed]["ric10"], ec.ric_true()))
    print(f"max angle(ric, truth) after min_frames pushes {worst:.3e} deg")
    assert worst <= MARGIN * RIC_MEASURED_DEG


def test_rc_is_the_true_relative_rotation(runs):
    """guards against the wrong one of R1 / R2 / the transpose: any of them is tens of degrees away"""
    worst, chosen = 0.0, set()
    for seed in SEEDS:
        for pr, row in zip(runs[seed]["pushes"], runs[seed]["rows"]):
            assert row["flags"] == er.SOLVED and row["count"] == 40
            worst = max(worst, ec.angle_between(row["Rc"], pr["Rc"]))
            chosen.add(row["chosen"])
    print(f"max angle(Rc, truth) {worst:.3e} deg; chosen {sorted(chosen)}")
    assert worst <= MARGIN * RC_MEASURED_DEG
    assert chosen == {0, 1}


def test_one_axis_rotation_never_succeeds():
    cal = er.Calibrator(n_hypotheses=K)
    for pr in ec.make_pushes(7, 14, one_axis=True):
        row = cal.push(pr["a"], pr["b"], pr["dq"])
        assert not row["ok"] and row["sigma"][2] < 0.25
    print("one axis: sigma", row["sigma"])
    assert row["sigma"][1] > 0.25 and row["sigma"][2] < 1e-3          # two directions of the quaternion stay free


def test_sums_in_the_texts_order_and_kept_entries(runs):
    """G of the restatement (np.cumsum) against the sums written out term by term, and keep=True (the entries of earlier pushes kept) against computing all anew"""
    cal = runs[0]["cal"]
    _, _, B, G = cal.system()
    for p in range(4):
        for q in range(p, 4):
            acc = np.float64(0.0)
            for i in range(len(B)):
                for r in range(4):
                    acc = acc + B[i, r, p] * B[i, r, q]
            assert G[p, q] == acc and G[q, p] == acc
    kept = er.Calibrator(keep=True, n_hypotheses=K, seed=0)
    for pr, row in zip(runs[0]["pushes"], runs[0]["rows"]):
        got = kept.push(pr["a"], pr["b"], pr["dq"])
        assert all(np.array_equal(np.asarray(got[k]), np.asarray(row[k])) for k in row)


def test_atan2p_against_numpy():
    """the grid holds 0, equal arguments and the neighbourhood of 5 degrees (the half angle 2.5 degrees of the Huber switch)"""
    ys = np.concatenate([[0.0], np.linspace(0.0, 1.0, 2001), np.tan(np.deg2rad(np.linspace(2.4, 2.6, 401)))])
    worst = 0.0
    assert er.atan2p(0.0, 0.0) == 0.0
    for y in ys:
        for x in (0.0, 1.0, y, 0.5, 1e-9, 3.0):
            if x == 0.0 and y == 0.0:
                continue
            worst = max(worst, abs(er.atan2p(y, x) - np.arctan2(y, x)))
    print(f"max |atan2p - arctan2| {worst:.3e}")
    assert worst <= 4 * np.finfo(np.float64).eps                      # measured 4.4e-16 = 2 eps: a few roundings of a value below pi / 2
    assert er.atan2p(1.0, 1.0) == np.arctan2(1.0, 1.0) and er.atan2p(1.0, 0.0) == er.HALF_PI


def test_huber_weight_of_an_identity_pair():
    cal = er.Calibrator(n_hypotheses=K)
    pr = ec.make_pushes(11, 1, m=8, deg=20.0)[0]
    row = cal.push(pr["a"], pr["b"], pr["dq"])
    assert row["flags"] == 0 and row["best_k"] == -1 and np.array_equal(row["Rc"], np.eye(3))
    assert abs(row["angle"] - 20.0) < 1e-9 and row["weight"] == np.float64(5.0) / row["angle"]
    small = er.Calibrator(n_hypotheses=K)
    pr = ec.make_pushes(12, 1, deg=5.0)[0]
    row = small.push(pr["a"], pr["b"], pr["dq"])
    assert 0.0 < row["angle"] < 5.0 and row["weight"] == 1.0


def _manager(spans):
    f = sequence.FeatureManager()
    for fid, (start, n) in enumerate(spans):
        it = sequence.FeaturePerId(fid, start, -1.0)
        for k in range(n):
            it.feature_per_frame.append(sequence.FeaturePerFrame(np.array([fid + 0.1 * (start + k), -fid - 0.01 * (start + k), 1.0, 0, 0, 0, 0, -1.0]), 0.0))
        f.feature.append(it)
    return f


def test_get_corresponding():
    # (start_frame, observations): spans both; starts after l; ends before r; starts at l, ends at r; spans both again; ends at l
    f = _manager([(0, 6), (4, 3), (1, 3), (3, 2), (2, 5), (0, 4)])
    a, b = f.get_corresponding(3, 4)
    assert a.shape == b.shape == (3, 3)
    ids = [0, 3, 4]                                           # feature order
    assert np.array_equal(a, np.array([[i + 0.1 * 3, -i - 0.01 * 3, 1.0] for i in ids]))
    assert np.array_equal(b, np.array([[i + 0.1 * 4, -i - 0.01 * 4, 1.0] for i in ids]))
    a, b = f.get_corresponding(7, 8)
    assert a.shape == b.shape == (0, 3)


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.EXROT_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ['  printf("%d\\n%d\\n", VILF_EXROT_MAX_SLOTS, VILF_EXROT_MAX_HISTORY);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(checks) + 2
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out) if int(o) != e]
    assert not bad, bad
    assert [int(out[-2]), int(out[-1])] == [abi.VILF_EXROT_MAX_SLOTS, abi.VILF_EXROT_MAX_HISTORY] == [er.MAX_SLOTS, er.MAX_HISTORY]


def _options(estimate_extrinsic):
    from vil_fusion_amd.lib import default_options
    o = default_options()
    o.estimate_extrinsic = estimate_extrinsic
    return o


def _feed(est, case, k):
    for dt, acc, gyr in case["imu"][k]:
        est.process_imu(dt, acc, gyr)
    return est.prepare_image(case["images"][k], case["stamps"][k])


def test_gate_holds_the_initialisation_until_the_calibration_succeeds():
    """estimator.cpp:159-182. min_frames = 13 puts the first success three frames past the first full window (frame 10), so the gate has something to hold"""
    W, MIN_FRAMES = sequence.WINDOW_SIZE, 13
    case = ec.make_images(5, MIN_FRAMES + 3)
    backend = er.Backend(n_hypotheses=K, min_frames=MIN_FRAMES)
    est = sequence.SlidingWindowEstimator(_options(2), backend)
    assert est.estimate_extrinsic == 2
    for k in range(MIN_FRAMES):                               # frames 0 .. 12: pushes 1 .. 12, the window is full from frame 10 on
        assert _feed(est, case, k) is False
        assert est.solver_flag == est.INITIAL and est.estimate_extrinsic == 2 and est.events[-1] == "fill"
        assert est.frame_count == min(k + 1, W)
        assert backend.cal.frame_count == k
    assert np.array_equal(est.ric, np.array(est.o.RIC[:]).reshape(3, 3))
    assert est.ex_calibrated is None
    # frame 13: push 13 succeeds, and the same full window initialises
    assert _feed(est, case, MIN_FRAMES) is True
    row = est.ex_rows[-1]
    assert row["ok"] and row["frame_count"] == MIN_FRAMES and len(est.ex_rows) == MIN_FRAMES
    assert est.estimate_extrinsic == 1 and est.solver_flag == est.NON_LINEAR
    assert np.array_equal(est.ric, row["ric"]) and np.array_equal(est.ric, backend.cal.ric)
    assert est.ex_calibrated == (MIN_FRAMES, W)
    # the images hold the exact rotations and the IMU samples integrate to them up to the mid-point rule's error: 20 steps of at most 1 degree, each off by about
    # theta^3 / 12 = 4.4e-7 rad, in sum 8.9e-6 rad = 5.1e-4 deg per pair; added to the float32 points' error (RIC_MEASURED_DEG), with the same margin
    err = ec.angle_between(est.ric, ec.ric_true())
    print(f"angle(ric, truth) through the estimator {err:.3e} deg")
    assert err <= MARGIN * (5.1e-4 + RIC_MEASURED_DEG)
    # the calibrator is no longer pushed, and clear_state leaves it and the calibrated rotation alone
    est.clear_state()
    assert est.estimate_extrinsic == 1 and np.array_equal(est.ric, row["ric"]) and backend.cal.frame_count == MIN_FRAMES


def test_without_the_calibration_the_first_full_window_initialises():
    case = ec.make_images(5, sequence.WINDOW_SIZE + 1)
    backend = er.Backend(n_hypotheses=K)
    est = sequence.SlidingWindowEstimator(_options(1), backend)
    for k in range(sequence.WINDOW_SIZE):
        assert _feed(est, case, k) is False
    assert _feed(est, case, sequence.WINDOW_SIZE) is True
    assert backend.cal.frame_count == 0 and est.ex_rows == [] and est.estimate_extrinsic == 1
