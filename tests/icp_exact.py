"""An exact Umeyama step for the loop ICP (TEST INFRASTRUCTURE) and the clouds of tests/test_loop_icp_edges.py.

exact_step states one ICP step from its definition in mpmath at 60 digits: exact means, the centred cross-covariance H = sum (t - mean_t)(s - mean_s)^T / n (no raw
sums, so nothing cancels far from the origin), mp.svd_r, R = U diag(1, 1, det U det V) V^T, t = mean_t - R mean_s. It shares no arithmetic with icp_reference.umeyama64
(fp64 raw sums + LAPACK) or with icp_step / icp_rotation of vilf_icp.hip (fp64 raw sums + one-sided Jacobi).

Every cloud built here consists of float32 points that lie at least 1 m apart, so each falls into a 0.4 m leaf of its own and the voxel filter returns the cloud
unchanged as a set (in ascending leaf index). `filtered` asserts that on icp_reference.submap before anything else is done with a cloud."""
import functools
import math

import mpmath as mp
import numpy as np

import icp_reference as R

DPS = 60
F = np.float32
U32 = float(np.spacing(F(1.0)))          # one float32 spacing at 1


def _hp(fn):
    """run at 60 digits without touching the process-wide mp context"""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return wrapped


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0]) + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


@_hp
def exact_step(S, T):
    """float32 correspondences S[i] <-> T[i] -> dict(R (3, 3) fp64, t (3,) fp64, sigma: the three singular values of H in descending order, sign: det U det V,
    mean_s, mean_t (fp64))"""
    S, T = np.asarray(S, dtype=F)[:, :3], np.asarray(T, dtype=F)[:, :3]
    n = len(S)
    assert n == len(T) and n >= 1
    s = [[mp.mpf(float(v)) for v in row] for row in S]
    t = [[mp.mpf(float(v)) for v in row] for row in T]
    ms = [mp.fsum(r[k] for r in s) / n for k in range(3)]
    mt = [mp.fsum(r[k] for r in t) / n for k in range(3)]
    H = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            H[i, j] = mp.fsum((t[a][i] - mt[i]) * (s[a][j] - ms[j]) for a in range(n)) / n
    U, sig, V = mp.svd_r(H)                                  # H = U diag(sig) V: V is already the transpose
    sign = 1 if _det3(U) * _det3(V) > 0 else -1
    Rm = U * mp.diag([1, 1, sign]) * V
    tv = mp.matrix(mt) - Rm * mp.matrix(ms)
    return dict(R=np.array([[float(Rm[i, j]) for j in range(3)] for i in range(3)]), t=np.array([float(tv[i]) for i in range(3)]),
                sigma=[float(sig[k]) for k in range(3)], sign=sign, mean_s=np.array([float(v) for v in ms]), mean_t=np.array([float(v) for v in mt]))


@_hp
def exact_mse(d2):
    """the exact mean of the float d2 values, rounded once to fp64"""
    d2 = np.asarray(d2, dtype=F)
    return float(mp.fsum(mp.mpf(float(v)) for v in d2) / len(d2))


@_hp
def mse_error_in_units(mse, d2):
    """|mse - exact mean of the float d2| in units of 2^-53 x the exact mean, evaluated in mp against the unrounded mean (inf if the mean is 0 and mse is not)"""
    d2 = np.asarray(d2, dtype=F)
    m = mp.fsum(mp.mpf(float(v)) for v in d2) / len(d2)
    err = abs(mp.mpf(float(mse)) - m)
    if m == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / (m * mp.mpf(2) ** -53))


# ---- clouds -----------------------------------------------------------------------------------------------------------------------
def pad(c):
    c = np.asarray(c, dtype=F).reshape(-1, 3)
    return np.column_stack([c, np.zeros(len(c), dtype=F)]).astype(F)


def filtered(cloud, p=None):
    """the sub-map of the one cloud under the identity pose; asserts that the voxel filter kept every point as it was"""
    cloud = pad(np.asarray(cloud)[:, :3]) if len(cloud) else np.zeros((0, 4), dtype=F)
    out = R.submap([cloud], np.zeros((1, 6)), 0, 0, 0, p)
    assert len(out) == len(cloud), (len(out), len(cloud))
    assert {tuple(v) for v in out[:, :3]} == {tuple(v) for v in cloud[:, :3]}
    if len(cloud) > 1:
        from scipy.spatial import cKDTree
        assert cKDTree(cloud[:, :3].astype(np.float64)).query(cloud[:, :3].astype(np.float64), k=2)[0][:, 1].min() >= 1.0
    return out


def rot(rpy):
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])


def moved(pts, rpy, shift, about=None):
    """rotated by Rz Ry Rx about `about` (default: the centroid) and shifted, in fp64, then rounded to float"""
    p = np.asarray(pts, dtype=np.float64)[:, :3]
    c = p.mean(0) if about is None else np.asarray(about, dtype=np.float64)
    return ((p - c) @ rot(rpy).T + c + np.asarray(shift, dtype=np.float64)).astype(F)


RPY, SHIFT = (0.01, -0.02, 0.05), (0.2, -0.1, 0.05)


def lattice36(origin=(0.0, 0.0, 0.0), nx=6, ny=6):
    """nx x ny = 36 points 5 m apart, z in {0, 0.25, .., 1} by a fixed pattern that leaves the cloud of full rank"""
    assert nx * ny == 36
    z = [0.25 * ((3 * i + 2 * j + i * j) % 5) for j in range(ny) for i in range(nx)]
    xy = [(5.0 * i, 5.0 * j) for j in range(ny) for i in range(nx)]
    return (np.array([[x, y, zz] for (x, y), zz in zip(xy, z)], dtype=np.float64) + np.asarray(origin, dtype=np.float64)).astype(F)


STEP_CASES = ["generic", "far", "planar_target", "planar_both", "mirrored", "mirrored_tall", "three", "collinear", "one_target"]
FULL_CASES = STEP_CASES[:7]                # compared with the exact R and t; the last two: invariants only


def step_clouds(name):
    """(target, source, parameter overrides) of a case of the one-step test, as float (n, 4) clouds"""
    tg = lattice36()
    over = {}
    if name == "generic":
        src = moved(tg, RPY, SHIFT)
    elif name == "far":                                       # 5 km from the origin: the raw-sum form sum t s^T / n - mean_t mean_s^T cancels here
        off = np.array([5000.0, -3000.0, 40.0])
        src = (moved(tg, RPY, SHIFT).astype(np.float64) + off).astype(F)      # float + small integers: exact for x, y; z + 40 rounds, the cloud is what it is
        tg = (tg.astype(np.float64) + off).astype(F)
    elif name == "planar_target":                             # a wall seen from a tilted sensor: sigma_3 = 0, the rotation is still unique
        src = moved(tg, RPY, SHIFT)
        tg = tg.copy(); tg[:, 2] = 0.75
    elif name == "planar_both":
        tg = tg.copy(); tg[:, 2] = 0.75
        src = moved(tg, (0.0, 0.0, 0.05), (0.2, -0.1, 0.0))
        src[:, 2] = 0.75
    elif name in ("mirrored", "mirrored_tall"):               # the best orthogonal fit is a reflection: det U det V = -1
        # the square lattice has sigma_1 = sigma_2, so which column the Jacobi sweeps leave in front is open; on the 4 x 9 lattice the y column is the larger one and
        # the sort by singular value swaps two columns of V: there the sign factor of icp_rotation is -1
        tg = tg if name == "mirrored" else lattice36(nx=4, ny=9)
        m = tg.astype(np.float64).copy()
        m[:, 2] = 0.5 - m[:, 2]
        src = moved(m, (0.0, 0.0, 0.05), (0.0, 0.0, 0.0), about=tg.astype(np.float64).mean(0))
    elif name == "three":                                     # three centred points are coplanar: rank two by construction; a fourth just outside the gate
        keep = [1, 16, 32]
        src = np.concatenate([moved(tg, RPY, SHIFT)[keep], (tg[keep[0]].astype(np.float64) + [3.0, -4.0, 0.125])[None, :].astype(F)])
        tg = tg[keep]
        over = dict(max_correspondence_distance=5.0)
    elif name == "collinear":                                 # 12 points 3 m apart along (2, 2, 1) / 3, the source 0.25 m beside them
        k = np.arange(12, dtype=np.float64)[:, None]
        tg = (k * np.array([2.0, 2.0, 1.0]) + np.array([1.0, -3.0, 0.5])).astype(F)
        src = (tg.astype(np.float64) + np.array([0.0, 0.25, 0.0])).astype(F)
    elif name == "one_target":
        tg = np.array([[3.0, -2.0, 1.0]], dtype=F)
        src = (tg.astype(np.float64) + np.array([[1.5, 0.0, 0.25], [-1.0, 2.0, 0.0], [0.5, -2.5, 1.0], [-2.0, -1.0, -0.75]])).astype(F)
    else:
        raise KeyError(name)
    return pad(tg), pad(src), over


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(F)).astype(np.float64)


def step_case(name):
    """everything the one-step test knows before the device is looked at: the filtered clouds S, T, the restatement's one round and its correspondences, the exact step
    on those correspondences, the restatement's own fp64 distance from it (both summation orders) and, for the cases compared in full, the tolerance per entry"""
    tg, src, over = step_clouds(name)
    p = R.Params(max_iterations=1, history_keyframes=0, **over)
    S, T = filtered(src, p), filtered(tg, p)
    ref = R.align(S, T, p)
    idx, d2 = ref["first_search"]
    ok = (idx >= 0) & (d2.astype(np.float64) <= p.max_correspondence_distance ** 2)
    Ss, Ts = S[ok, :3], T[idx[ok], :3]
    assert ref["iterations"] == 1 and ref["criterion"] == R.ITERATIONS and ref["converged"] and ref["n_correspondences"] == int(ok.sum()) >= 3
    ex = exact_step(Ss, Ts)
    r64 = [R.umeyama64(Ss, Ts, rev) for rev in (False, True)]
    c = dict(name=name, over=over, params=p, tgt=tg, src=src, S=S, T=T, ref=ref, ok=ok, Ss=Ss, Ts=Ts, exact=ex, mse=exact_mse(d2[ok]), n=int(ok.sum()))
    if name in FULL_CASES:
        # the rotation is determined: sigma_2 well above zero (a condition on the inputs, not a measurement)
        assert ex["sigma"][1] / ex["sigma"][0] > 1e-6, ex["sigma"]
        c["dist_R"] = max(float(np.abs(Rm - ex["R"]).max()) for Rm, _ in r64)
        c["dist_t"] = max(float(np.abs(tv - ex["t"]).max()) for _, tv in r64)
        # one float32 spacing at the exact entry (two fp64 values closer than half a spacing can round to neighbouring floats) + 10 x the restatement's own distance
        c["tol"] = np.column_stack([ulp32(ex["R"]) + 10.0 * c["dist_R"], ulp32(ex["t"]) + 10.0 * c["dist_t"]])
    else:
        # R is not determined below rank two. What is: R mean_s + t = mean_t. The restatement's own residual of it, in mp from its fp64 R and t:
        c["dist_t"] = max(float(np.abs(residual_of_means(Rm, tv, ex)).max()) for Rm, tv in r64)
        if name == "collinear":
            d = (Ts[-1].astype(np.float64) - Ts[0]) / np.linalg.norm(Ts[-1].astype(np.float64) - Ts[0])
            ds = (Ss[-1].astype(np.float64) - Ss[0]) / np.linalg.norm(Ss[-1].astype(np.float64) - Ss[0])
            c["dir_t"], c["dir_s"] = d, ds
            c["dist_dir"] = max(float(np.abs(Rm @ ds - d).max()) for Rm, _ in r64)
    return c


@_hp
def residual_of_means(Rm, tv, ex):
    """R mean_s + t - mean_t of a given R (3, 3) and t (3,) (any float type), evaluated in mp"""
    ms, mt = [mp.mpf(float(v)) for v in ex["mean_s"]], [mp.mpf(float(v)) for v in ex["mean_t"]]
    return np.array([float(mp.fsum([mp.mpf(float(Rm[i][j])) * ms[j] for j in range(3)] + [mp.mpf(float(tv[i])), -mt[i]])) for i in range(3)])


def means_tolerance(c):
    """bound of |R mean_s + t - mean_t| per component for a float R and t. The tolerance of a translation entry (one float32 spacing at its magnitude + 10 x the
    restatement's own residual), with the magnitude of t bounded by |mean_t| + |mean_s| (t = mean_t - R mean_s, R a rotation), plus what rounding R itself to float
    moves R mean_s by: half a spacing at 1 per entry times |mean_s_j|. Every term comes from the inputs and the number formats."""
    ex = c["exact"]
    return ulp32(np.abs(ex["mean_t"]) + np.linalg.norm(ex["mean_s"])) + 0.5 * U32 * np.abs(ex["mean_s"]).sum() + 10.0 * c["dist_t"]


# ---- the grown grid -----------------------------------------------------------------------------------------------------------------
def grid_cell(T):
    """the sizing rule of DESIGN section 3g in float32: cells of 1.6 m, times 1.25 until prod(floor(extent / cell) + 1) <= 2^18 -> (cell, growths)"""
    ext = (T[:, :3].max(0) - T[:, :3].min(0)).astype(F)
    cell, grown = F(4.0) * F(0.4), 0
    while int(np.prod([int(np.floor(e / cell)) + 1 for e in ext], dtype=np.int64)) > (1 << 18):
        cell = F(cell * F(1.25))
        grown += 1
    return cell, grown


def big_scene(seed=11):
    """target: a jittered 16 m lattice over 1000 m x 1000 m x 40 m with an empty corridor 425 <= x < 575; source: queries beside target points, queries in the corridor
    at graded distances from its edges, and a few outside the target's box. All coordinates are multiples of 1/8 m."""
    rng = np.random.default_rng(seed)
    q8 = lambda a: np.round(np.asarray(a) * 8.0) / 8.0
    g = np.arange(4.0, 1000.0, 16.0)
    X, Y = np.meshgrid(g, g, indexing="ij")
    t = np.column_stack([X.ravel() + q8(rng.uniform(-4, 4, X.size)), Y.ravel() + q8(rng.uniform(-4, 4, X.size)), q8(rng.uniform(0, 40, X.size))])
    t = t[(t[:, 0] < 425.0) | (t[:, 0] >= 575.0)]
    t[0], t[1] = [0.0, 0.0, 0.0], [1000.0, 1000.0, 40.0]                       # the box
    tgt = t[rng.permutation(len(t))]
    u = rng.standard_normal((420, 3))
    reach = np.where(np.arange(420) < 300, rng.uniform(0.25, 3.0, 420), rng.uniform(6.5, 11.5, 420))      # most within the first shell, 120 reach into the second
    near = tgt[rng.choice(len(tgt), 420, replace=False)] + q8(u / np.linalg.norm(u, axis=1)[:, None] * reach[:, None])
    y = np.arange(10.0, 990.0, 2.5)[:360]
    e = q8(np.linspace(1.0, 74.0, len(y)))[rng.permutation(len(y))]            # distance from the corridor's edge
    side = rng.integers(0, 2, len(y))
    corridor = np.column_stack([np.where(side == 0, 425.0 + e, 575.0 - e), y, q8(rng.uniform(0, 40, len(y)))])
    outside = np.array([[-30.0 - 4.0 * k, 100.0 * k + 7.0, 20.0] for k in range(10)] + [[300.0 + 40.0 * k, 1020.0 + 8.0 * k, -10.0 - 5.0 * k] for k in range(10)])
    src = np.concatenate([near, corridor, outside])
    return pad(tgt.astype(F)), pad(src[rng.permutation(len(src))].astype(F))


def line_scene():
    """target: 200 points 2 m apart along x (a grid of N x 1 x 1 cells); queries beside, above and beyond it, out to the whole-target scan"""
    tgt = np.array([[2.0 * k - 50.0, 3.0, 1.0] for k in range(200)], dtype=F)
    q = []
    for k in range(60):
        d = 0.25 * 1.12 ** k                                                    # 0.25 m .. 200 m
        d = round(d * 8.0) / 8.0
        q.append([-45.0 + 6.5 * k, 3.0 + (d if k % 2 else 0.0), 1.0 + (0.0 if k % 2 else -d)])
    q += [[-80.0, 3.0, 1.0], [-52.5, 4.0, 1.0], [349.0, 3.0, 2.0], [420.0, -30.0, 1.0]]
    return pad(tgt), pad(np.array(q, dtype=F))


def point_scene():
    """target: one point (one cell); queries from 0 m to 150 m away"""
    tgt = np.array([[7.0, -2.0, 1.5]], dtype=F)
    q = [[7.0, -2.0, 1.5]] + [[7.0 + 1.5 * k, -2.0 - 2.0 * (k % 3), 1.5 + 0.5 * k] for k in range(1, 12)] + [[157.0, -2.0, 1.5], [7.0, -102.0, 21.5]]
    return pad(tgt), pad(np.array(q, dtype=F))


# ---- gate, criteria, sizes ------------------------------------------------------------------------------------------------------------
def gate_scene(drop_one=False):
    """max_correspondence_distance = 5. Source 0 sits exactly (3, 4, 0) from target 0: d2 == 25.0f, accepted. Source 1 sits (3, -4 - one float32 spacing of 8, 0) from
    target 1, whose y is 8 + one spacing: d2 > 25, rejected. Sources 2 and 3 are accepted; drop_one leaves 2 correspondences."""
    y1 = np.nextafter(F(8.0), F(9.0))
    tgt = np.array([[0.0, 0.0, 0.0], [20.0, y1, 0.0], [40.0, 0.0, 2.0], [0.0, 30.0, 1.0]], dtype=F)
    src = np.array([[3.0, 4.0, 0.0], [23.0, 4.0, 0.0], [40.5, 0.25, 2.0], [-0.25, 30.5, 1.25]], dtype=F)
    return pad(tgt), pad(src[:3] if drop_one else src)


def noisy_source(tg, seed=3):
    """the generic motion plus a per-point offset of up to 3/64 m: the mse settles at a floor above zero"""
    rng = np.random.default_rng(seed)
    return (moved(tg, RPY, SHIFT).astype(np.float64) + rng.integers(-3, 4, (len(tg), 3)) / 64.0).astype(F)


TREE_SIZES = [3, 63, 64, 65, 255, 256, 257, 512, 513]


def tree_scene(seed=0):
    """one 600-point target (30 x 20 points 2 m apart, z by a pattern) and eleven sources: lattices of exactly TREE_SIZES points (the first ns target points, moved a
    little and jittered by up to 1/16 m), one with 2 correspondences (and three points far outside the 3 m gate) and an empty one -> (clouds, pairs, parameter overrides)"""
    rng = np.random.default_rng(seed)
    tg = np.array([[2.0 * i, 2.0 * j, 0.25 * ((2 * i + 3 * j + i * j) % 7)] for j in range(20) for i in range(30)], dtype=F)
    order = rng.permutation(len(tg))
    clouds = [pad(tg)]
    for k, ns in enumerate(TREE_SIZES):
        sub = tg[np.sort(order[:ns])] if ns > 3 else tg[[31, 215, 400]]
        s = moved(sub, (0.004, -0.003, 0.01 + 0.002 * k), (0.1, -0.05 - 0.01 * k, 0.03), about=tg.astype(np.float64).mean(0)).astype(np.float64)
        clouds.append(pad((s + rng.integers(-4, 5, s.shape) / 64.0).astype(F)))
    clouds.append(pad(np.array([[10.25, 10.0, 0.5], [20.0, 30.25, 1.0], [200.0, 0.0, 0.0], [0.0, 300.0, 0.0], [-150.0, -100.0, 5.0]], dtype=F)))
    clouds.append(np.zeros((0, 4), dtype=F))
    pairs = [(0, k) for k in range(1, len(clouds))]
    return clouds, pairs, dict(history_keyframes=0, max_iterations=3, max_correspondence_distance=3.0)
