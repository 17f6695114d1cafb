"""tests/kfloop_reference.py, the numpy restatement of the second stage of the visual loop closure, measured against things that are not the restatement: scipy's
least squares on the correspondences the scene knows to be true, scipy's rotations for the decision, and the sampler's and the gate's own properties. No GPU."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation
import kfloop_reference as kl
import kfloop_cases as kc
from vil_fusion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (460.0, 460.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)
THR = 10.0 / 460.0
OFFSETS = [(5.0, 1.0), (15.0, 3.0), (25.0, 5.0)]
SEEDS = [1, 2]
# the largest difference between the restatement's refitted pose and scipy's over the six recovery scenes, measured on the CPU: 8.5e-11 rad and 1.9e-9 m (ten
# damped iterations from the winner against a converged trust region). The tolerance is ten times that; it may not be looser than 1e-4 rad or 1e-4 m and is not.
POSE_TOL_RAD, POSE_TOL_M = 8.5e-10, 1.9e-8


def store():
    return kl.KeyFrameStore(640, 480, CAM, None, cap_keyframes=64)


@pytest.mark.parametrize("m", [5, 6, 26, 1000])
def test_sampler_draws_distinct_members(m):
    for seed in (0, 7, 0xffffffff):
        S = kl.samples(m, 512, seed)
        assert S.shape == (512, 5) and S.min() >= 0 and S.max() < m
        assert all(len(set(row)) == 5 for row in S.tolist())
    assert not np.array_equal(kl.samples(m, 64, 1), kl.samples(m, 64, 2)) or m == 5
    if m == 1000:
        assert len(np.unique(kl.samples(m, 512, 3))) > 800          # the draws cover the members


def scipy_fit(X, u, R0, t0):
    """least squares on the normalised reprojection error from (R0, t0), a rotation vector on the left of R0 -> (R, t)"""
    X, u = X.astype(np.float64), u.astype(np.float64)

    def res(x):
        p = X @ (Rotation.from_rotvec(x[:3]).as_matrix() @ R0).T + x[3:]
        return (p[:, :2] / p[:, 2:3] - u).ravel()

    sol = least_squares(res, np.concatenate([np.zeros(3), t0]), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return Rotation.from_rotvec(sol.x[:3]).as_matrix() @ R0, sol.x[3:]


def recovery(seed, deg, trans):
    sc = kc.scene(seed, 80, [dict(m=60, outliers=0.4, deg=deg, trans=trans, noise=1.0)])
    st = store()
    cur, olds = kc.load(st, sc, check=st)
    row = st.findConnection(cur, olds, sc["qic"], sc["tic"])[0]
    return sc, sc["olds"][0], row


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("deg,trans", OFFSETS)
def test_recovers_the_true_correspondences_and_their_pose(seed, deg, trans):
    sc, o, row = recovery(seed, deg, trans)
    X, u = sc["cur"]["point_3d"][o["members"]], o["u"]
    assert o["true"].sum() == 36 and row["n_matched"] == 60
    R, t = scipy_fit(X[o["true"]], u[o["true"]], o["R_true"], o["t_true"])
    p = X.astype(np.float64) @ R.T + t
    err = np.sqrt(((p[:, :2] / p[:, 2:3] - u) ** 2).sum(axis=1))
    want = (p[:, 2] > 0) & (err <= THR)
    borderline = np.abs(err - THR) <= 0.05 * THR
    got = row["status"][o["members"]].astype(bool)
    assert np.array_equal(got[~borderline], want[~borderline]), np.flatnonzero(got != want)
    assert np.array_equal(want[~borderline], o["true"][~borderline])                  # every true correspondence, and no other
    assert row["flags"] == kl.REFIT | kl.LOOP and row["has_loop"] and row["n_inliers"] == got.sum()
    d_rot = np.linalg.norm(Rotation.from_matrix(row["R"] @ R.T).as_rotvec())
    d_t = np.linalg.norm(row["t"] - t)
    print(f"seed {seed} offset {deg} deg / {trans} m: refit against scipy {d_rot:.3e} rad, {d_t:.3e} m; inliers {got.sum()}")
    assert np.array_equal(got, o["true"])             # no borderline member in these scenes: the two fits are of the same set
    assert d_rot <= POSE_TOL_RAD and d_t <= POSE_TOL_M
    # the decision sees the offset the scene put in
    assert abs(np.linalg.norm(row["relative_t"]) - trans) < 0.2 and abs(row["relative_yaw"]) < deg + 0.5


def random_rotations(n, seed):
    return Rotation.random(n, random_state=seed).as_matrix()


def test_decision_against_scipy_rotations():
    rng = np.random.default_rng(5)
    mats = list(random_rotations(40, 3))
    # every branch of the quaternion rule: traces <= 0 around each axis
    mats += [Rotation.from_rotvec(np.pi * 0.999 * a).as_matrix() for a in np.eye(3)] + [Rotation.from_rotvec(3.0 * np.array(a) / np.linalg.norm(a)).as_matrix() for a in ([1, 2, 3], [3, 1, 2], [2, 3, 1])]
    branches = set()
    for i, P in enumerate(mats):
        Rv, PT, Tv = mats[(i * 7 + 3) % len(mats)], rng.uniform(-5, 5, 3), rng.uniform(-5, 5, 3)
        rt, q, yaw, _ = kl.decide(P, PT, Rv, Tv)
        M = P.T @ Rv
        branches.add("trace" if np.trace(M) > 0 else int(np.argmax(np.diag(M))))
        ref = Rotation.from_matrix(M).as_quat()                                  # (x, y, z, w), sign free
        ref = np.array([ref[3], ref[0], ref[1], ref[2]])
        assert np.abs(q - ref * np.sign(q @ ref)).max() < 1e-12 and abs(np.linalg.norm(q) - 1) < 1e-12
        assert np.abs(rt - Rotation.from_matrix(P).inv().apply(Tv - PT)).max() < 1e-12
        y0, y1 = Rotation.from_matrix(Rv).as_euler("ZYX", degrees=True)[0], Rotation.from_matrix(P).as_euler("ZYX", degrees=True)[0]
        d = y0 - y1
        assert abs(((yaw - d) + 180.0) % 360.0 - 180.0) < 1e-12 and -180.0 <= yaw <= 180.0       # degrees
        assert abs(kl.yaw_deg(Rv) - y0) < 1e-12
    assert branches == {"trace", 0, 1, 2}


def test_normalize_angle_at_the_edges():
    assert kl.normalize_angle(180.0) == -180.0 and kl.normalize_angle(-180.0) == 180.0           # the reference's floor rule, as it stands
    assert kl.normalize_angle(180.0 - 1e-9) == 180.0 - 1e-9 and kl.normalize_angle(-180.0 + 1e-9) == -180.0 + 1e-9          # (within an ulp of 180 the quotient rounds to 1)
    assert abs(kl.normalize_angle(180.0 + 1e-9) - (-180.0 + 1e-9)) < 1e-13 and abs(kl.normalize_angle(-180.0 - 1e-9) - (180.0 - 1e-9)) < 1e-13
    assert kl.normalize_angle(0.0) == 0.0 and kl.normalize_angle(359.0) == -1.0 and kl.normalize_angle(-359.0) == 1.0 and kl.normalize_angle(190.0) == -170.0


def test_decision_thresholds_from_both_sides():
    eps = 1e-6
    for yaw, dist, want in ((30.0 - eps, 1.0, True), (30.0 + eps, 1.0, False), (-(30.0 - eps), 1.0, True), (-(30.0 + eps), 1.0, False), (1.0, 20.0 - eps, True), (1.0, 20.0 + eps, False)):
        P = kc.rot([0, 0, 1], 20.0)
        Rv = kc.rot([0, 0, 1], 20.0 + yaw)
        PT = np.array([1.0, -2.0, 0.5])
        Tv = PT + dist * np.array([2.0, -1.0, 2.0]) / 3.0
        rt, _, y, loop = kl.decide(P, PT, Rv, Tv)
        assert abs(y - yaw) < 1e-9 and abs(np.linalg.norm(rt) - dist) < 1e-9 and loop == want, (yaw, dist, y, loop)
        assert kl.decide(P, PT, Rv, Tv, max_yaw=abs(yaw) + 2 * eps, max_dist=dist + 2 * eps)[3]


def test_gate_at_min_loop_num():
    for m, pnp in ((25, False), (26, True)):
        sc = kc.scene(4, 40, [dict(m=m, outliers=0, deg=5.0, trans=1.0)])
        st = store()
        cur, olds = kc.load(st, sc, check=st)
        row = st.findConnection(cur, olds, sc["qic"], sc["tic"], n_hypotheses=64)[0]
        assert row["n_matched"] == m
        if pnp:
            assert row["flags"] == kl.REFIT | kl.LOOP and row["n_inliers"] == 26 and row["status"].sum() == 26 and row["loop_info"].shape == (8,)
        else:
            assert row["flags"] == kl.GATE and row["n_inliers"] == 0 and not row["status"].any() and not row["R"].any() and row["loop_info"] is None and not row["has_loop"]


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.KFL_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ['  printf("%d %d %d %d %d\\n", VILF_KFL_GATE, VILF_KFL_NO_HYPOTHESIS, VILF_KFL_REFIT, VILF_KFL_REFIT_DROPPED, VILF_KFL_LOOP);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[-5:]] == [abi.VILF_KFL_GATE, abi.VILF_KFL_NO_HYPOTHESIS, abi.VILF_KFL_REFIT, abi.VILF_KFL_REFIT_DROPPED, abi.VILF_KFL_LOOP]
    assert [kl.GATE, kl.NO_HYPOTHESIS, kl.REFIT, kl.REFIT_DROPPED, kl.LOOP] == [int(v) for v in out[-5:]]
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out[:-5]) if int(o) != e]
    assert len(out) - 5 == len(checks) and not bad, bad
