"""Scan-to-map association: an independent restatement and an exact reference (numpy + mpmath only).

Written from the reference's text — EstimationMapping.hpp: pointAssociaToMap (:355), EdgeCostFactor (:117), SurfCostFactor (:174) — and from the
documented behaviour of what it calls (pcl::KdTreeFLANN::nearestKSearch with FLANN's L2_Simple in float, Eigen's SelfAdjointEigenSolver and
ColPivHouseholderQR), not from oracle/scan2map.cpp and not from the kernels.

Two tiers:
  * the FLOAT RULE (`associate`): every rounding the reference performs is performed — the query in double then float, squared distances
    (ex*ex + ey*ey) + ez*ez with every operation rounded to float32, equal distances keep the lower map index, the gate d2[4] < 1.0f, the
    fits in double;
  * the EXACT TIER (`exact_query`): rational distances, mpmath (60 digits) for the eigen problem and the least squares. Per query it says which
    decisions are DECIDED — the exact quantity is further from its threshold than 64 x the bound on the evaluated quantity's own rounding
    error (DESIGN 3k's convention) — and returns the exact line direction / plane with the tolerances derived below.
"""
from fractions import Fraction
import numpy as np
import mpmath as mp

DPS = 60                    # digits of the exact tier (set per call: mp.workdps)
F32 = np.float32
U32 = 2.0 ** -24            # unit roundoff, float32
EPS = 2.0 ** -52            # machine epsilon, double (Eigen's NumTraits<double>::epsilon())
SAFETY = 64.0
UNDECIDED_BOUND = 1e-3
NONE_D2 = F32(3.0e38)


# ---------------------------------------------------------------------------------------------------------------- float rule
def transform(pose_qt, pts_xyz):
    """pointAssociaToMap: Eigen's q * v (v + w * 2(u x v) + u x 2(u x v)) + t in double, stored in a float point."""
    q = np.asarray(pose_qt, dtype=np.float64)
    u, w, t = q[:3], q[3], q[4:7]
    v = np.asarray(pts_xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    uv = 2.0 * np.cross(np.broadcast_to(u, v.shape), v)
    pw = v + w * uv + np.cross(np.broadcast_to(u, v.shape), uv)
    return (pw + t).astype(np.float32)


def sqdist_f32(map_xyz, q):
    """FLANN L2_Simple on floats: every subtraction, product and sum rounded to float32."""
    m = np.asarray(map_xyz, dtype=np.float32)
    ex = m[:, 0] - F32(q[0]); ey = m[:, 1] - F32(q[1]); ez = m[:, 2] - F32(q[2])
    return (ex * ex + ey * ey) + ez * ez


def knn5(map_xyz, q):
    """Linear scan in map (PCL index) order; of equal distances the lower index stays in front. Fewer than five points: index -1, 3e38."""
    idx = np.full(5, -1, dtype=np.int64); d2 = np.full(5, NONE_D2, dtype=np.float32)
    if len(map_xyz) == 0:
        return idx, d2
    d = sqdist_f32(map_xyz, q)
    order = np.argsort(d, kind="stable")[:5]
    idx[:len(order)] = order; d2[:len(order)] = d[order]
    return idx, d2


def line_fit(nb):
    """EdgeCostFactor :131-157. nb: (5, 3) doubles. -> (valid, pa, pb, w, cov, center)"""
    center = np.zeros(3)
    for j in range(5):
        center = center + nb[j]
    center = center / 5.0
    cov = np.zeros((3, 3))
    for j in range(5):
        z = nb[j] - center
        cov = cov + np.outer(z, z)
    w, V = np.linalg.eigh(cov)              # ascending
    direction = V[:, 2]
    valid = bool(w[2] > 3 * w[1])
    return valid, 0.1 * direction + center, -0.1 * direction + center, w, cov, center


def _householder(x):
    """Eigen makeHouseholder: H x = beta e0, H = I - tau v v^T, v = (1, essential)."""
    c0 = x[0]; tail = x[1:]
    tsq = float(np.dot(tail, tail))
    if tsq <= np.finfo(np.float64).tiny:
        return 0.0, c0, np.zeros_like(tail)
    beta = np.sqrt(c0 * c0 + tsq)
    if c0 >= 0:
        beta = -beta
    return (beta - c0) / beta, beta, tail / (c0 - beta)


def colpiv_qr_solve(A, b):
    """Eigen::ColPivHouseholderQR<Matrix<double,5,3>>::solve: pivot on the largest remaining column norm, rank = #{|R_kk| > eps * 3 * max|R_kk|},
    x = P [R11^-1 (Q^T b)_1 ; 0]."""
    A = np.array(A, dtype=np.float64); c = np.array(b, dtype=np.float64)
    rows, cols = A.shape
    perm = list(range(cols)); maxpivot = 0.0
    for k in range(cols):
        norms = [float(np.dot(A[k:, j], A[k:, j])) for j in range(k, cols)]
        p = k + int(np.argmax(norms))
        if p != k:
            A[:, [k, p]] = A[:, [p, k]]; perm[k], perm[p] = perm[p], perm[k]
        tau, beta, ess = _householder(A[k:, k])
        A[k, k] = beta; A[k + 1:, k] = 0.0
        maxpivot = max(maxpivot, abs(beta))
        v = np.concatenate([[1.0], ess])
        if tau != 0.0:
            for j in range(k + 1, cols):
                A[k:, j] -= tau * v * float(np.dot(v, A[k:, j]))
            c[k:] -= tau * v * float(np.dot(v, c[k:]))
    thresh = EPS * min(rows, cols) * maxpivot
    rank = sum(1 for k in range(cols) if abs(A[k, k]) > thresh)        # (the pivots come in non-increasing order up to rounding)
    z = np.zeros(cols)
    for k in range(rank - 1, -1, -1):
        z[k] = (c[k] - float(np.dot(A[k, k + 1:rank], z[k + 1:rank]))) / A[k, k]
    x = np.zeros(cols)
    for k in range(cols):
        x[perm[k]] = z[k]
    return x, rank


def plane_fit(nb):
    """SurfCostFactor :187-213. -> (valid, n, d, x, rank)"""
    x, rank = colpiv_qr_solve(nb, -np.ones(5))
    with np.errstate(all="ignore"):
        nrm = np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        d = 1.0 / nrm
        n = x / nrm
        valid = True
        for j in range(5):
            if np.abs(n[0] * nb[j, 0] + n[1] * nb[j, 1] + n[2] * nb[j, 2] + d) > 0.2:
                valid = False
                break
    return bool(valid), n, d, x, rank


def fit_is_robust(nb, is_surf):
    """Is the fit's yes/no the same in every correct double evaluation? Only a threshold decision that sits inside the evaluation's own error is not: the exact
    tier's margins (64 x the bound), evaluated in double, for w2 against 3 w1 and for each residual against 0.2. A covariance that is exactly diagonal has its
    diagonal as eigenvalues in any solver: its comparison is exact whatever the margin. A plane whose fit is UNDECIDED (the derived bound exceeds 1e-3: rank
    deficient or nearly so) has no usable bound on its residuals; there the kind is compared all the same, as for every other undecided fit."""
    pmax = float(np.abs(nb).max())
    with np.errstate(all="ignore"):
        if not is_surf:
            _, _, _, w, cov, center = line_fit(nb)
            if cov[0, 1] == 0 and cov[0, 2] == 0 and cov[1, 2] == 0:
                return True
            dmax = float(np.abs(nb - center).max())
            bw = 3.0 * (5 * 2 * dmax * 4 * EPS * pmax) + 8 * EPS * float(np.linalg.norm(cov))
            return bool(abs(w[2] - 3 * w[1]) > SAFETY * 4 * bw)
        s = np.linalg.svd(nb, compute_uv=False)
        if not s[2] > s[0] * 1e-13:
            return True
        ok, n, d, x, rank = plane_fit(nb)
        kappa = s[0] / s[2]
        tol0 = EPS * (kappa + kappa ** 2 * np.linalg.norm(nb @ x + 1) / (s[0] * np.linalg.norm(x)))
        if not SAFETY * tol0 <= UNDECIDED_BOUND:
            return True
        bres = 2 * tol0 * (3 * pmax + d) + 4 * EPS * (3 * pmax + d)
        for j in range(5):
            res = abs(n @ nb[j] + d)
            if not abs(res - 0.2) > SAFETY * bres:
                return False
            if res > 0.2:
                break
        return True


def associate(map_xyz, queries_xyz, pose_qt, is_surf):
    """The float rule for a whole query cloud. -> dict of arrays: q (float), idx (nq, 5), d2 (nq, 5), kind (0 / 1 edge / 2 surf), rec (nq, 6)."""
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3])
    q = transform(pose_qt, np.asarray(queries_xyz, dtype=np.float32)[:, :3])
    nq = len(q)
    out = dict(q=q, idx=np.full((nq, 5), -1, dtype=np.int64), d2=np.full((nq, 5), NONE_D2, dtype=np.float32), kind=np.zeros(nq, dtype=np.int32), rec=np.zeros((nq, 6)),
               robust=np.ones(nq, dtype=bool))
    if len(m) < 5:
        return out
    for i in range(nq):
        idx, d2 = knn5(m, q[i])
        out["idx"][i] = idx; out["d2"][i] = d2
        if not d2[4] < F32(1.0):
            continue
        nb = m[idx].astype(np.float64)
        out["robust"][i] = fit_is_robust(nb, is_surf)
        if not is_surf:
            ok, pa, pb = line_fit(nb)[:3]
            if ok:
                out["kind"][i] = 1; out["rec"][i, :3] = pa; out["rec"][i, 3:] = pb
        else:
            ok, n, d = plane_fit(nb)[:3]
            if ok:
                out["kind"][i] = 2; out["rec"][i, :3] = n; out["rec"][i, 3] = d
    return out


# ---------------------------------------------------------------------------------------------------------------- exact tier
def _frac3(p):
    return [Fraction(float(p[0])), Fraction(float(p[1])), Fraction(float(p[2]))]


def exact_neighbours(map_xyz, q):
    """The six smallest exact squared distances (rationals) to the float query q, with their indices (ties: lower index first)."""
    m64 = np.asarray(map_xyz, dtype=np.float32).astype(np.float64)
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    d = ((m64 - q64) ** 2).sum(1)                         # relative error <= a few 2^-53: only a pre-selection
    k = min(len(d), 6)
    kth = np.partition(d, k - 1)[k - 1]
    cand = np.nonzero(d <= kth * (1 + 1e-9) + 1e-300)[0]
    fq = _frac3(q64)
    ex = []
    for j in cand:
        fm = _frac3(m64[j])
        ex.append((sum((a - b) ** 2 for a, b in zip(fm, fq)), int(j)))
    ex.sort()
    return ex[:6]


GAMMA5 = 5 * U32 / (1 - 5 * U32)       # |fl(d2) - d2| <= GAMMA5 * d2: three rounded differences squared (1+u)^2, a rounded product, two rounded sums of non-negative terms


def exact_query(map_xyz, q, is_surf):
    """exact_tier_query at DPS digits, whatever precision the caller's mpmath context has"""
    with mp.workdps(DPS):
        return _exact_query(map_xyz, q, is_surf)


def _exact_query(map_xyz, q, is_surf):
    """Exact tier for ONE float query q against the map. -> dict:
       idx (the exact five, ascending distance), dec_set / dec_gate / dec_fit (booleans: the decision is decided), gate (exact), and for the fit:
       edge: valid (exact w2 > 3 w1), dir (unit, exact), center, tol_dir, fit_decided (tolerance below UNDECIDED_BOUND)
       surf: valid (all exact residuals <= 0.2), x (the exact least-squares solution), n, d, tol_rel, dec_res[5], fit_decided"""
    m = np.asarray(map_xyz, dtype=np.float32)
    r = dict(dec_set=False, dec_gate=False, dec_fit=False, fit_decided=False, gate=False, valid=False, idx=None)
    if len(m) < 5:
        return r
    ex = exact_neighbours(m, q)
    d5 = ex[4][0]
    r["idx"] = [j for _, j in ex[:5]]
    if len(ex) < 6:
        r["dec_set"] = True
    else:
        d6 = ex[5][0]
        r["dec_set"] = float(d6 - d5) > SAFETY * GAMMA5 * float(d5 + d6)
    # the order inside the list is part of "the neighbours, in list order": every adjacent pair must be decided too
    for a, b in zip(ex[:4], ex[1:5]):
        if not float(b[0] - a[0]) > SAFETY * GAMMA5 * float(a[0] + b[0]):
            r["dec_order"] = False
    r.setdefault("dec_order", True)
    r["gate"] = d5 < 1
    r["dec_gate"] = abs(float(d5 - 1)) > SAFETY * GAMMA5 * float(d5)
    if not r["gate"]:
        r["dec_fit"] = True          # nothing is fitted
        return r
    P = [[mp.mpf(Fraction(float(v)).numerator) / mp.mpf(Fraction(float(v)).denominator) for v in m[j, :3]] for j in r["idx"]]
    pmax = max(abs(float(v)) for j in r["idx"] for v in m[j, :3])
    if not is_surf:
        c = [sum(P[j][a] for j in range(5)) / 5 for a in range(3)]
        Z = [[P[j][a] - c[a] for a in range(3)] for j in range(5)]
        cov = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                cov[a, b] = sum(Z[j][a] * Z[j][b] for j in range(5))
        w, V = mp.eigsy(cov)
        order = sorted(range(3), key=lambda k: w[k])
        w = [w[k] for k in order]
        cf = mp.sqrt(sum(cov[a, b] ** 2 for a in range(3) for b in range(3)))
        dmax = max(abs(float(z)) for row in Z for z in row)
        # error of the evaluated covariance: the centred coordinates carry 4 eps pmax (centroid: four sums and a division at magnitude <= 5 pmax, /5; one
        # subtraction), each of the 5 products of an entry 2 dmax times that, the sums another 8 eps of the entry; the eigenvalues move by at most its norm (Weyl)
        bw = 3.0 * (5 * 2 * dmax * 4 * EPS * pmax) + 8 * EPS * float(cf)
        r["valid"] = bool(w[2] > 3 * w[1])
        r["dec_fit"] = abs(float(w[2] - 3 * w[1])) > SAFETY * 4 * bw
        gap = w[2] - w[1]
        r["w"] = [float(x) for x in w]
        r["center"] = np.array([float(x) for x in c])
        r["dir"] = np.array([float(V[a, order[2]]) for a in range(3)])
        r["cov_f"] = float(cf)
        r["tol_dir"] = float(SAFETY * EPS * cf / gap) if gap > 0 else float("inf")
        r["fit_decided"] = r["tol_dir"] <= UNDECIDED_BOUND
        r["pmax"] = pmax
    else:
        A = mp.matrix(5, 3)
        for j in range(5):
            for a in range(3):
                A[j, a] = P[j][a]
        b = mp.matrix([-1] * 5)
        S = mp.svd_r(A, compute_uv=False)
        smax, smin = max(S), min(S)
        r["pmax"] = pmax
        if smin <= smax * mp.mpf(10) ** -25:
            r["kappa"] = float("inf"); r["tol_rel"] = float("inf"); r["dec_fit"] = False
            return r
        kappa = smax / smin
        x = mp.lu_solve(A.T * A, A.T * b)                 # 60 digits: the squared condition number costs at most 50 of them here (smin/smax > 1e-25)
        res = A * x - b
        xn = mp.norm(x); rn = mp.norm(res)
        tol0 = EPS * (kappa + kappa ** 2 * rn / (smax * xn))
        r["kappa"] = float(kappa); r["tol_rel"] = float(SAFETY * tol0)
        r["fit_decided"] = r["tol_rel"] <= UNDECIDED_BOUND
        d = 1 / xn
        n = x / xn
        r["x"] = np.array([float(v) for v in x]); r["n"] = np.array([float(v) for v in n]); r["d"] = float(d)
        resid = [abs(sum(n[a] * P[j][a] for a in range(3)) + d) for j in range(5)]
        # the evaluated residual: n and d carry the relative error tol0 of x (twice for the direction after normalisation), the dot product 4 eps of its terms
        bres = [float(2 * tol0) * (3 * pmax + float(d)) + 4 * EPS * (3 * pmax + float(d)) for _ in range(5)]
        r["resid"] = [float(v) for v in resid]
        r["dec_res"] = [abs(float(resid[j]) - 0.2) > SAFETY * bres[j] for j in range(5)]
        thr = mp.mpf("0.200000000000000011102230246251565404236316680908203125")        # the double 0.2
        first_bad = next((j for j in range(5) if resid[j] > thr), 5)
        r["valid"] = first_bad == 5
        # the loop breaks at the first failing residual: only the residuals up to it take part in the decision
        r["dec_fit"] = all(r["dec_res"][:min(first_bad + 1, 5)]) and r["fit_decided"]
    return r


def pair_error(pa, pb, ra, rb):
    """distance between the unordered pairs {pa, pb} and {ra, rb} (the eigenvector's sign is free)"""
    e1 = max(np.abs(pa - ra).max(), np.abs(pb - rb).max())
    e2 = max(np.abs(pa - rb).max(), np.abs(pb - ra).max())
    return min(e1, e2)


def line_points_tolerance(ex):
    """Tolerance on the line's two points: they sit 0.1 along the direction (0.1 x the direction's tolerance) at the centroid, which is itself a rounded
    double at the neighbours' magnitude (64 eps pmax: the same factor over the sums' rounding)."""
    return 0.1 * ex["tol_dir"] + SAFETY * EPS * max(ex["pmax"], 1.0)


def rule_tolerances(nb, is_surf):
    """The derived tolerances evaluated in double from the five neighbours (for comparing two double evaluations with each other: twice the bound). -> (tol, pmax);
    tol = inf when the fit is undecided."""
    pmax = max(float(np.abs(nb).max()), 1.0)
    with np.errstate(all="ignore"):
        if not is_surf:
            _, _, _, w, cov, _ = line_fit(nb)
            gap = w[2] - w[1]
            tol_dir = SAFETY * EPS * np.linalg.norm(cov) / gap if gap > 0 else np.inf
            return (2 * (0.1 * tol_dir + SAFETY * EPS * pmax) if tol_dir <= UNDECIDED_BOUND else np.inf), pmax
        s = np.linalg.svd(nb, compute_uv=False)
        if s[2] <= s[0] * 1e-13:
            return np.inf, pmax
        x = np.linalg.lstsq(nb, -np.ones(5), rcond=None)[0]
        kappa = s[0] / s[2]
        tol = SAFETY * EPS * (kappa + kappa ** 2 * np.linalg.norm(nb @ x + 1) / (s[0] * np.linalg.norm(x)))
        return (2 * tol if tol <= UNDECIDED_BOUND else np.inf), pmax


def record_error(kind, rec, ref_rec):
    """edge: the unordered pair {pa, pb}; surf: the relative error of the un-normalised solution x = n / d"""
    if kind == 1:
        return pair_error(rec[:3], rec[3:6], ref_rec[:3], ref_rec[3:6])
    x, xr = rec[:3] / rec[3], ref_rec[:3] / ref_rec[3]
    return float(np.linalg.norm(x - xr) / np.linalg.norm(xr))



# ---------------------------------------------------------------------------------------------------------------- the cell arithmetic (host restatement)
LOFF = 65536
QR = F32(1.001)
DMARGIN = 8


def cell_shift(leaf, half=100.0):
    cs = 0
    while cs < 15 and (float(F32(leaf)) * (1 << cs) < 0.5 or 2.0 * half / (float(F32(leaf)) * (1 << cs)) + 2.0 + 2 * DMARGIN > 512.0):
        cs += 1
    return cs


def cell_of(v, leaf, cs):
    """floor(v * inv) + 65536 >> cs with the product in float32"""
    inv = F32(1.0) / F32(leaf)
    return (np.floor(np.asarray(v, dtype=np.float32) * inv).astype(np.int64) + LOFF) >> cs


def query_rows(q, leaf, cs):
    """-> cylo, nrow, cxlo, cxhi1 of a float query"""
    qx, qy = F32(q[0]), F32(q[1])
    cylo = int(cell_of(qy - QR, leaf, cs)); nrow = int(cell_of(qy + QR, leaf, cs)) - cylo + 1
    cxlo = int(cell_of(qx - QR, leaf, cs)); cxhi1 = int(cell_of(qx + QR, leaf, cs)) + 1
    return cylo, nrow, cxlo, cxhi1


def candidates_per_row(map_xyz, q, leaf, cs):
    """how many map points each row of the query's span holds (what the walk visits when the directory is right)"""
    m = np.asarray(map_xyz, dtype=np.float32)
    cylo, nrow, cxlo, cxhi1 = query_rows(q, leaf, cs)
    cx = cell_of(m[:, 0], leaf, cs); cy = cell_of(m[:, 1], leaf, cs)
    return [int(((cy == cylo + r) & (cx >= cxlo) & (cx < cxhi1)).sum()) for r in range(nrow)]
