"""Scalar restatement of include/vilfusion.h, "Feature manager: triangulate": Python floats (IEEE fp64, one rounding per operation, no fused multiply-add), every
sum in the stated order. TEST INFRASTRUCTURE: the device path is compared with this to the bit, and this with the oracle's FeatureManager::triangulate to the bit
(test_feature_triangulate.py)."""
import math
import numpy as np

USED, DONE, RESET, NONFINITE = 1, 2, 4, 8
SWEEPS = 60
INF, NAN = float("inf"), float("nan")


def div(a, b):
    """a / b as IEEE has it where Python raises"""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def sqrt(x):
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def sum3(a0, b0, a1, b1, a2, b2):
    """the sum from 0.0 of three products"""
    return ((0.0 + a0 * b0) + a1 * b1) + a2 * b2


def cameras(Ps, Rs, tic, ric):
    """paragraph "camera": per frame (tc [3], Rc [9])"""
    Ps = np.asarray(Ps, dtype=np.float64).reshape(-1, 3).tolist()
    Rs = np.asarray(Rs, dtype=np.float64).reshape(-1, 9).tolist()
    tic = np.asarray(tic, dtype=np.float64).reshape(3).tolist()
    ric = np.asarray(ric, dtype=np.float64).reshape(9).tolist()
    cams = []
    for P, R in zip(Ps, Rs):
        tc = [P[r] + dot3(R[3 * r], tic[0], R[3 * r + 1], tic[1], R[3 * r + 2], tic[2]) for r in range(3)]
        Rc = [sum3(R[3 * r], ric[q], R[3 * r + 1], ric[3 + q], R[3 * r + 2], ric[6 + q]) for r in range(3) for q in range(3)]
        cams.append((tc, Rc))
    return cams


def design_matrix(cams, start, points):
    """paragraph "design matrix": the rows of A as lists of 4"""
    t0, R0 = cams[start]
    A = []
    for o, (x, y, z) in enumerate(points):
        tj, Rj = cams[start + o]
        d = [tj[e] - t0[e] for e in range(3)]
        t = [dot3(R0[r], d[0], R0[3 + r], d[1], R0[6 + r], d[2]) for r in range(3)]
        R = [sum3(R0[r], Rj[c], R0[3 + r], Rj[3 + c], R0[6 + r], Rj[6 + c]) for r in range(3) for c in range(3)]
        P = [[R[3 * c + r] for c in range(3)] + [-dot3(R[r], t[0], R[3 + r], t[1], R[6 + r], t[2])] for r in range(3)]
        n = sqrt((x * x + y * y) + z * z)
        f0, f1, f2 = div(x, n), div(y, n), div(z, n)
        A.append([f0 * P[2][c] - f2 * P[0][c] for c in range(4)])
        A.append([f1 * P[2][c] - f2 * P[1][c] for c in range(4)])
    return A


def smallest_right_singular_vector(A):
    """paragraph "right singular vector" -> (v [4], sweeps). A is changed in place"""
    rows = len(A)
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    sweeps = 0
    for _ in range(SWEEPS):
        rotated = False
        sweeps += 1
        for p in range(3):
            for q in range(p + 1, 4):
                alpha = beta = gamma = 0.0
                for r in range(rows):
                    ap, aq = A[r][p], A[r][q]
                    alpha += ap * ap; beta += aq * aq; gamma += ap * aq
                if abs(gamma) <= 1e-17 * sqrt(alpha * beta) or gamma == 0.0:
                    continue
                rotated = True
                zeta = div(beta - alpha, 2.0 * gamma)
                t = div(1.0 if zeta >= 0 else -1.0, abs(zeta) + sqrt(1.0 + zeta * zeta))
                c = div(1.0, sqrt(1.0 + t * t))
                s = c * t
                for M in (A, V):
                    for row in M:
                        ap, aq = row[p], row[q]
                        row[p] = c * ap - s * aq
                        row[q] = s * ap + c * aq
        if not rotated:
            break
    best, bound = 0, INF
    for c in range(4):
        n = 0.0
        for r in range(rows):
            n += A[r][c] * A[r][c]
        if n < bound:
            bound, best = n, c
    return [V[i][best] for i in range(4)], sweeps


def is_used(n_obs, start, window_size=10):
    return n_obs >= 2 and start < window_size - 2


def triangulate(table, window_size=10, init_depth=5.0):
    """the whole call for one table (FeatureManager.triangulation_table's dict) -> dict(depth, inv_depth, flags, sweeps, result) as estimator.triangulate_features"""
    start, first = np.asarray(table["start_frame"], dtype=np.int64), np.asarray(table["first_obs"], dtype=np.int64)
    pts = np.asarray(table["points"], dtype=np.float64).reshape(-1, 3)
    din = np.asarray(table["depth"], dtype=np.float64)
    n = len(start)
    cams = None
    depth, flags, sweeps, inv = din.copy(), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), []
    res = dict(n_used=0, n_candidates=0, n_reset=0, n_nonfinite=0)
    for f in range(n):
        nobs = int(first[f + 1] - first[f])
        if not is_used(nobs, int(start[f]), window_size):
            continue
        flags[f] = USED
        res["n_used"] += 1
        d = float(din[f])
        if not d > 0:
            if cams is None:
                cams = cameras(table["Ps"], table["Rs"], table["tic"], table["ric"])
            v, sw = smallest_right_singular_vector(design_matrix(cams, int(start[f]), pts[first[f]:first[f + 1]].tolist()))
            d = div(v[2], v[3])
            flags[f] |= DONE
            res["n_candidates"] += 1
            if d < 0.1:
                d = init_depth
                flags[f] |= RESET
                res["n_reset"] += 1
            if math.isinf(d) or d != d:
                flags[f] |= NONFINITE
                res["n_nonfinite"] += 1
            depth[f], sweeps[f] = d, sw
        inv.append(div(1.0, d) if d > 0 else div(1.0, init_depth))
    return dict(depth=depth, inv_depth=np.array(inv, dtype=np.float64), flags=flags, sweeps=sweeps, result=res)


def design_matrix_of(table, f):
    """the design matrix of feature f of a table as an array (for the comparison with np.linalg.svd)"""
    first = np.asarray(table["first_obs"], dtype=np.int64)
    pts = np.asarray(table["points"], dtype=np.float64).reshape(-1, 3)
    return np.array(design_matrix(cameras(table["Ps"], table["Rs"], table["tic"], table["ric"]), int(table["start_frame"][f]), pts[first[f]:first[f + 1]].tolist()))
