"""The graphs of the 4-DoF pose-graph tests (TEST INFRASTRUCTURE): the small cases measured against tests/pg4_exact.py, the reject case, the layout edges and
the two laps of the end-to-end test. Everything is generated from fixed seeds; nothing here looks at the code under test.

A case is a dict(vio_R [n][3][3], vio_T [n][3], sequence [n], fixed [n], loops [(from, to, rel_t [3], rel_yaw)], params {overrides})."""
import functools
import math

import numpy as np

import pg4_exact
import pg4_reference as ref


def trajectory(n, seed, pitch=2.0, roll=-1.5, yaw_start=10.0, yaw_step=7.0, step=1.0, yaw_drift=0.4, t_drift=0.03):
    """ground truth on a gentle curve and a VIO copy of it that drifts in yaw and translation: -> gt (yaw [n], t [n][3]), vio_R, vio_T"""
    rng = np.random.default_rng(seed)
    gy = np.array([ref.normalize_angle(yaw_start + yaw_step * k) for k in range(n)])
    gt = np.zeros((n, 3))
    for k in range(1, n):
        gt[k] = gt[k - 1] + step * np.array([math.cos(gy[k - 1] * ref.D2R), math.sin(gy[k - 1] * ref.D2R), 0.05 * math.sin(0.7 * k)])
    vy = np.array([ref.normalize_angle(gy[k] + yaw_drift * k + 0.1 * rng.standard_normal()) for k in range(n)])
    vt = gt + np.cumsum(t_drift * rng.standard_normal((n, 3)) + t_drift, axis=0)
    vt[0] = gt[0]
    pk = pitch + 0.5 * rng.standard_normal(n)
    rk = roll + 0.5 * rng.standard_normal(n)
    vio_R = np.array([ref.ypr2R(vy[k], pk[k], rk[k]) for k in range(n)])
    return (gy, gt, pk, rk), vio_R, vt


def gt_loop(gt, a, b, rng, noise_t=0.02, noise_yaw=0.3):
    gy, gtt, pk, rk = gt
    Ra = ref.ypr2R(gy[a], pk[a], rk[a])
    return (a, b, Ra.T @ (gtt[b] - gtt[a]) + noise_t * rng.standard_normal(3), ref.normalize_angle(gy[b] - gy[a]) + noise_yaw * rng.standard_normal())


def make(n, seed, pairs, sequence=None, fixed=None, params=None, **kw):
    gt, vio_R, vio_T = trajectory(n, seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    sequence = list(sequence) if sequence is not None else [1] * n
    fixed = list(fixed) if fixed is not None else [1] + [0] * (n - 1)
    return dict(vio_R=vio_R, vio_T=vio_T, sequence=sequence, fixed=fixed, loops=[gt_loop(gt, a, b, rng) for (a, b) in pairs], params=dict(params or {}), gt=gt)


def vio_loop(c, a, b, offset):
    """a loop whose residual at the start is exactly `offset` along x (translation) and 0 in yaw, to rounding"""
    ypr_a = ref.R2ypr(c["vio_R"][a])
    ypr_b = ref.R2ypr(c["vio_R"][b])
    Ra = ref.ypr2R(*ypr_a)
    return (a, b, Ra.T @ (c["vio_T"][b] - c["vio_T"][a]) - np.array([offset, 0.0, 0.0]), ref.normalize_angle(ypr_b[0] - ypr_a[0]))


@functools.lru_cache(maxsize=None)
def small_cases():
    C = {}
    C["three_loops"] = make(12, 1, [(0, 11), (2, 9), (2, 10)])
    C["in_band"] = make(12, 2, [(5, 7)])
    C["repeated"] = make(12, 3, [(1, 10), (1, 10)])
    C["shared_old"] = make(12, 4, [(1, 9), (1, 10)])
    # 178.25 .. 182.1: both sides of the wrap. The loops are made strong (yaw scale 1, Huber out of reach) so that the yaw corrections are some hundredths of a degree;
    # node 5 starts 0.01 degrees above -180 and its first update carries it across
    C["wrap"] = make(12, 5, [(1, 10), (3, 8)], yaw_start=178.25, yaw_step=0.3, yaw_drift=0.05, params=dict(loop_yaw_scale=1.0, huber=10.0))
    C["pitch_roll"] = make(12, 6, [(0, 11), (2, 9)], pitch=30.0, roll=-20.0)
    h = make(12, 7, [])
    h["loops"] = [vio_loop(h, 1, 9, 0.05), vio_loop(h, 2, 11, 3.0)]                                   # |r| = 0.05 (inside a = 0.1) and 3 (outside)
    C["huber"] = h
    C["two_sequences"] = make(12, 8, [(1, 8), (3, 10)], sequence=[1] * 6 + [2] * 6)
    C["sequence0_fixed"] = make(12, 9, [(1, 9), (2, 11)], sequence=[0] * 4 + [1] * 8, fixed=[1] * 4 + [0] * 8)
    C["n1"] = make(1, 10, [])
    C["n2"] = make(2, 11, [(0, 1)])
    C["no_loops"] = make(12, 12, [])
    C["max_iterations_0"] = make(12, 1, [(0, 11), (2, 9), (2, 10)], params=dict(max_iterations=0))
    return C


def reject_case():
    """a straight line of 12 nodes 200 m apart, one loop (1, 11) that asks for 150 degrees and (0, 2000, 0), Huber out of reach"""
    n = 12
    vio_R = np.array([np.eye(3)] * n)
    vio_T = np.array([[200.0 * k, 0.0, 0.0] for k in range(n)])
    return dict(vio_R=vio_R, vio_T=vio_T, sequence=[1] * n, fixed=[1] + [0] * (n - 1), loops=[(1, 11, np.array([0.0, 2000.0, 0.0]), 150.0)],
                params=dict(huber=1e6, min_relative_decrease=0.4))


def layout_cases():
    C = {}
    for n in (4, 5, 8, 9):
        C[f"n{n}"] = make(n, 20 + n, [(0, n - 1)])
    for n in (63, 64, 65, 129):
        C[f"n{n}"] = make(n, 20 + n, [(0, n - 1), (5, n - 7), (n // 2, n - 2)], yaw_step=360.0 / n)
    for L in (15, 16, 17, 31, 32, 33):
        C[f"L{L}"] = make(140, 200 + L, [(k, k + 7) for k in range(L)], yaw_step=2.0)
    C["sequence_at_group"] = make(24, 300, [(2, 20), (5, 13)], sequence=[1] * 12 + [2] * 12)          # the change falls on a group boundary
    C["sequence_after_group"] = make(24, 301, [(2, 20), (5, 14)], sequence=[1] * 13 + [2] * 11)      # and one node after it
    return C


def two_laps(n_lap=40, seed=77):
    """two laps of a square, n_lap key frames each; VIO drifts in yaw and translation; a loop for every third key frame of the second lap to the key frame at the
    same place in the first, from ground truth with noise"""
    n = 2 * n_lap
    rng = np.random.default_rng(seed)
    side = n_lap // 4
    gy, gt = np.zeros(n), np.zeros((n, 3))
    for k in range(1, n):
        gy[k] = ref.normalize_angle(90.0 * (((k - 1) % n_lap) // side))
        gt[k] = gt[k - 1] + 1.0 * np.array([math.cos(gy[k] * ref.D2R), math.sin(gy[k] * ref.D2R), 0.0])
    gy[0] = gy[n_lap]
    vy = np.array([ref.normalize_angle(gy[k] + 0.03 * k + 0.05 * rng.standard_normal()) for k in range(n)])
    vt = np.zeros((n, 3))
    for k in range(1, n):                       # odometry steps rotated by the yaw error: the drift of a real VIO
        dy = (vy[k - 1] - gy[k - 1]) * ref.D2R
        Rz = np.array([[math.cos(dy), -math.sin(dy), 0], [math.sin(dy), math.cos(dy), 0], [0, 0, 1]])
        vt[k] = vt[k - 1] + Rz @ (gt[k] - gt[k - 1]) + 0.005 * rng.standard_normal(3)
    pk, rk = 0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal(n)
    vio_R = np.array([ref.ypr2R(vy[k], pk[k], rk[k]) for k in range(n)])
    g = (gy, gt, pk, rk)
    loops = [gt_loop(g, k - n_lap, k, rng, 0.02, 0.2) for k in range(n_lap, n, 3)]
    return dict(vio_R=vio_R, vio_T=vt, sequence=[1] * n, fixed=[1] + [0] * (n - 1), loops=loops, params={}, gt=g)


def params_of(case, **over):
    P = ref.default_params()
    P.update(case["params"])
    P.update(over)
    return P


@functools.lru_cache(maxsize=None)
def exact(name, snapshots=(1, 2, 5)):
    """the exact run of a small case (or "reject"), once per process"""
    c = reject_case() if name == "reject" else small_cases()[name]
    P = params_of(c)
    if P["max_iterations"] == 0:
        snapshots = (0,)
    return pg4_exact.run(c["vio_R"], c["vio_T"], c["sequence"], c["fixed"], c["loops"], P, snapshots)


def check_margins(name, floor=1e-6):
    """no rho within `floor` (relative) of min_relative_decrease, no stop rule at equality, in the exact run of the case"""
    out = exact(name)
    for k, snap in out.items():
        for what, margin in snap["margins"]:
            assert margin > floor, (name, k, what, margin)


# ---- what the tests measure with -------------------------------------------------------------------------------------------------------------------------------------
def yaw_diff(a, b):
    """largest |a - b| in degrees, modulo a turn (179.99.. and -179.99.. are neighbours)"""
    d = np.asarray(a, float).reshape(-1) - np.asarray(b, float).reshape(-1)
    return float(np.max(np.abs((d + 180.0) % 360.0 - 180.0))) if d.size else 0.0


# What the restatement differs from the exact run by, measured on the CPU over every small case and the snapshots after 1, 2 and 5 attempts (one run each; the largest
# is sequence0_fixed after two attempts): 2.6e-14 m, 3.2e-13 degrees, 1.8e-13 relative in a cost. The reject case works at 2000 m: 1.9e-11 m, 9.7e-13 degrees.
MEASURED_T, MEASURED_YAW, MEASURED_COST = 2.6e-14, 3.2e-13, 1.8e-13
MEASURED_T_REJECT, MEASURED_YAW_REJECT = 1.9e-11, 9.7e-13
CPU_TOL = dict(t=max(10 * MEASURED_T, 1e-13), yaw=max(10 * MEASURED_YAW, 1e-12), cost=10 * MEASURED_COST)                 # ten times the measured figure, with the floors
CPU_TOL_REJECT = dict(t=10 * MEASURED_T_REJECT, yaw=10 * MEASURED_YAW_REJECT, cost=10 * MEASURED_COST)
GPU_TOL = dict(t=max(1e-11, 1000 * MEASURED_T), yaw=max(6e-11, 1000 * MEASURED_YAW), cost=1e-10)                           # the margin of DESIGN section 3h
GPU_TOL_REJECT = dict(t=1000 * MEASURED_T_REJECT, yaw=max(6e-11, 1000 * MEASURED_YAW_REJECT), cost=1e-10)
LAYOUT_TOL = dict(t=1e-10, yaw=6e-10)                                                                                      # device against the restatement, one attempt
EPS = 2.0 ** -52
COST_FLOOR = 1e-12           # costs are compared relative to max(|cost|, this): below it a cost is rounding noise of residuals that are zero (the graph without loops)


def rho_bound(row):
    """what rounding alone may change in rho = (cost - cost') / model: the numerator cancels. A residual is a difference of coordinates (up to 180 degrees, tens of
    metres) and carries their rounding, up to some hundred times its own; a cost sums some fifty blocks. So |d rho| <= 1000 EPS cost / |cost - cost'| max(1, |rho|).
    Not a measured figure: it follows from the number format and the size of the cases. mu is a function of rho with |d mu / mu| <= 18 |d rho| (the derivative of
    1 - (2 rho - 1)^3 is at most 6, the divisor at least 1 / 3): its bound is 20 times this."""
    cost, cost_c, rho = row[0], row[1], row[2]
    return 1e-12 if cost == cost_c else max(1e-12, 1000.0 * EPS * abs(cost) / abs(cost - cost_c) * max(1.0, abs(rho)))


def compare(out, snap):
    """a run (the restatement's or the device's dict) against a snapshot of the exact run -> dict of the figures: t (m), yaw (degrees), cost (relative), rho and mu
    as multiples of rho_bound. Decisions, counts and flags are asserted equal here."""
    res, H, E = out["result"], np.asarray(out["history"], float).reshape(-1, 5), snap["history"]
    assert res["iterations"] == snap["iterations"] and res["accepted"] == snap["accepted"], (res, snap["iterations"], snap["accepted"])
    assert res["flags"] == snap["flags"], (res["flags"], snap["flags"])
    assert H.shape == E.shape and np.array_equal(H[:, 4], E[:, 4]), (H, E)
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(b), COST_FLOOR))) if len(a) else 0.0
    bounds = np.array([rho_bound(r) for r in E])
    mu_after = np.append(H[1:, 3], res["radius"]) if len(H) else np.zeros(0)
    mu_exact = np.append(E[1:, 3], snap["radius"]) if len(E) else np.zeros(0)
    return dict(t=float(np.max(np.abs(np.asarray(out["t"]) - snap["t"]))), yaw=yaw_diff(np.asarray(out["ypr"])[:, 0], snap["yaw"]),
                cost=max(rel(H[:, 0], E[:, 0]), rel(H[:, 1], E[:, 1]), rel([res["cost0"], res["cost1"]], np.array([snap["cost0"], snap["cost1"]]))),
                rho=float(np.max(np.abs(H[:, 2] - E[:, 2]) / bounds)) if len(H) else 0.0,
                mu=float(np.max(np.abs(mu_after - mu_exact) / np.abs(mu_exact) / (20.0 * bounds))) if len(H) else 0.0)


def within(fig, tol):
    """the figures of compare() against a tolerance dict; rho and mu against their bound"""
    return fig["t"] <= tol["t"] and fig["yaw"] <= tol["yaw"] and fig["cost"] <= tol["cost"] and fig["rho"] <= 1.0 and fig["mu"] <= 1.0
