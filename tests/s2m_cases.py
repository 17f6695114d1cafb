"""Designed inputs for the scan-to-map association tests (tests/test_scan2map_association.py). Every case is one map and one query cloud (used as
the edge pair against the edge map and as the surf pair against the surf map unless it says otherwise), small enough for seconds, with a stated TARGET that
`check_target` asserts on the CPU through the host restatement of the cell arithmetic (s2m_reference.cell_of / query_rows / candidates_per_row).

group: "default" = leaves 0.4 / 0.8 (cells of 0.8 m for both maps), "small" = leaves 0.25 / 0.02 (cells of 0.5 m and 0.64 m: five and six rows, the walk's tail loop),
       "half" = leaves 0.5 / 0.5 (cells of 0.5 m; dyadic lattices with one point per leaf keep their exact ties through the voxel grid), "tiny" = default leaves, maps of 4..6 points.
tier:  "exact" = meant for the exact tier (the 90 % decided condition counts it), "float" = built to be undecided (ties, thresholds hit exactly, degenerate fits):
       the float rule checks it in full.
states: which map states the case runs in ("all", or ("init",) for maps that a voxel grid would change in kind: exact duplicates)."""
import numpy as np
import s2m_reference as R

F32 = np.float32
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
LEAVES = {"default": (0.4, 0.8), "small": (0.25, 0.02), "half": (0.5, 0.5)}
CELL = 0.8
WALK_TOTALS = (0, 1, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25)


def _xyzi(p):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.column_stack([p, np.ones(len(p))]).astype(np.float32)


def _case(name, group, tier, target, mp_, q, pose=IDENT, states="all", **kw):
    return dict(name=name, group=group, tier=tier, target=target, map=_xyzi(mp_) if np.asarray(mp_).shape[-1] == 3 else mp_, q=_xyzi(q) if np.asarray(q).shape[-1] == 3 else q,
                pose=np.asarray(pose, dtype=np.float64), states=states, **kw)


def _cluster(rng, centre, n, r=0.3):
    """n distinct points within r of centre, one per 1/64 lattice site (distinct floats, generic distances)"""
    pts = set()
    while len(pts) < n:
        o = np.round(rng.uniform(-r, r, 3) * 512) / 512
        pts.add(tuple(o))
    return np.array(sorted(pts)) + np.asarray(centre)


# ---------------------------------------------------------------------------------------------------------------- gate
def gate_cases():
    out = []
    one = F32(1.0)
    for tag, a in (("eq1", one), ("below1", np.nextafter(one, F32(0))), ("above1", np.nextafter(one, F32(2)))):
        a = float(a)
        m = [[a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, a], [7, 7, 7], [-7, -7, 3], [9, -9, 0]]
        out.append(_case("gate_" + tag, "default", "float", dict(kind="gate5", passes=tag == "below1"), m, [[0, 0, 0]]))
    # the same five at exactly 1 around a dyadic query away from the origin (the differences are exact)
    c = np.array([16.0, -16.0, 2.0])
    m = [c + o for o in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1])] + [[40, 40, 0], [-40, 3, 0]]
    out.append(_case("gate_eq1_far", "default", "float", dict(kind="gate5", passes=False), m, [c]))
    # five points of one plane (y = const, far from the origin) on an arc, each at FLOAT squared distance exactly 1.0: a line (w2 = 2 > 3 * 0.11) and a plane that would
    # both be accepted if the gate let them through
    c = np.array([8.0, -8.0, 3.0])
    arc = [_at_float_distance_one(c, o) for o in ([0.8, 0, -0.6], [-0.8, 0, -0.6], [0.6, 0, -0.8], [-0.6, 0, -0.8], [0.0, 0, -1.0])]
    out.append(_case("gate_eq1_arc", "default", "float", dict(kind="gate5", passes=False, fits=True), arc + [[40, 40, 0], [-40, 3, 0]], [c]))
    # a fifth neighbour 0.995 m away in the column (row) that only a search radius of at least 1 reaches: the cell edge lies between q -+ 0.99 and the neighbour
    m, qs = [], []
    for k, (axis, sgn) in enumerate(((0, -1), (0, 1), (1, -1), (1, 1))):
        E = np.array([20.0 * CELL * (k - 2), 16.0 * CELL, 0.0])              # a cell corner
        q = E + [0.4, 0.4, 0.4]
        q[axis] = E[axis] - sgn * 0.994
        far = q.copy(); far[axis] = E[axis] + sgn * 0.001
        o = [1, 0][axis]                                                     # the other horizontal axis
        near = []
        for a, d in ((o, 0.45), (o, -0.45), (2, 0.45), (2, -0.45)):
            pnt = q.copy(); pnt[a] += d; near.append(pnt)
        m += near + [far]; qs.append(q)
    out.append(_case("gate_radius_edge", "default", "exact", dict(kind="radius_edge"), m, qs))
    # the fifth neighbour in the next cell, between 1.0 and the search radius 1.001 away: found or not, the gate must fail
    q = np.array([0.75, 0.4, 0.0])                                     # cell 0 (0 .. 0.8); 0.75 + 1.0005 = 1.7505 -> cell 2
    m = [q + o for o in ([0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [-0.1, 0, 0.05], [1.0005, 0, 0], [-1.0007, 0, 0], [0, 1.0004, 0], [0, -1.0006, 0])] + [[30, 30, 0]]
    out.append(_case("gate_fifth_between", "default", "exact", dict(kind="fifth_between"), m, [q]))
    # queries on cell boundaries (and one float to either side), in x and y, on both sides of 0 — where the slot index wraps from 511 to 0
    rng = np.random.default_rng(11)
    m = _grid_cloud(rng, -4.0, 4.0, 0.35, zs=(-0.2, 0.3))
    qs = []
    for k in (-3, -2, -1, 0, 1, 2, 3):
        b = F32(k) * F32(CELL)
        for v in (np.nextafter(b, F32(-9)), b, np.nextafter(b, F32(9))):
            qs += [[v, F32(0.33), 0.05], [F32(-0.41), v, 0.05], [v, v, 0.0]]
    out.append(_case("gate_cell_boundaries", "default", "exact", dict(kind="boundaries"), m, qs))
    # q -+ 1.001 straddling a cell edge: neighbouring floats whose span starts (ends) one cell apart
    qs = []
    for edge in (-2.4, -0.8, 0.0, 0.8, 1.6):
        for sgn in (1.0, -1.0):
            q0 = F32(edge + sgn * 1.001)
            cand = [q0]
            for _ in range(6):
                cand = [np.nextafter(cand[0], F32(-99))] + cand + [np.nextafter(cand[-1], F32(99))]
            for v in cand:
                qs += [[v, F32(0.2), 0.0], [F32(-0.3), v, 0.1]]
    out.append(_case("gate_span_straddle", "default", "exact", dict(kind="straddle"), m, qs))
    return out


def _at_float_distance_one(c, o):
    """the float point nearest c + o (moved along z by a few floats) whose float squared distance to c is exactly 1.0f"""
    c32 = np.asarray(c, dtype=np.float32)
    p = (np.asarray(c) + np.asarray(o)).astype(np.float32)
    for x_steps in range(0, 40):
        px = p.copy()
        for _ in range(x_steps):
            px[0] = np.nextafter(px[0], F32(1e9))
        for direction in (F32(1e9), F32(-1e9)):
            t = px.copy()
            for _ in range(64):
                if R.sqdist_f32(t[None, :], c32)[0] == F32(1.0):
                    return t.astype(np.float64)
                t[2] = np.nextafter(t[2], direction)
    raise AssertionError("no float point at squared distance exactly 1")


def _grid_cloud(rng, lo, hi, step, zs=(0.0,), jitter=0.1):
    xs = np.arange(lo, hi + 1e-9, step)
    p = np.array([[x, y, z] for x in xs for y in xs for z in zs])
    return p + np.round(rng.uniform(-jitter, jitter, p.shape) * 1024) / 1024


# ---------------------------------------------------------------------------------------------------------------- candidate walk
ROW_OFF = (-0.95, -0.5, 0.2, 0.75)        # y offsets that land in rows 0..3 of a query at y = 0.8 k + 0.1 (four rows: k-2 .. k+1)
ROW_MASKS = ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 1, 1), (1, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 0))


def walk_case(group="default"):
    """isolated clusters of exactly T candidates, spread over chosen rows of a four-row span; the query sits at the cluster's centre.
    Clusters are 16 cells apart in x and 8 rows apart in y: no span sees two of them."""
    rng = np.random.default_rng(5)
    pts, qs, want = [], [], []
    slot = 0
    plan = [(T, mask, None) for T in WALK_TOTALS for mask in (ROW_MASKS[:6] if T not in (5, 8, 9, 17) else ROW_MASKS)]
    plan += [(5, (0, 0, 1, 0), (-7, -7)), (5, (0, 0, 1, 0), (7, 3))]          # the map's first and last cell (cell-major order): their points are some query's five
    for T, mask, at in plan:
        rows = [r for r in range(4) if mask[r]]
        if T < len(rows) and T > 0:
            rows = rows[:T]
        kx, ky = at if at else ((slot % 12) - 6, (slot // 12) - 6)
        slot += 1
        c = np.array([kx * 16 * CELL + 0.4, ky * 8 * CELL + 0.1 + (0.19 * (slot % 3) if group == "small" else 0.0), 0.5])      # small cells: several phases, five and six rows
        per = [T // len(rows) + (1 if i < T % len(rows) else 0) for i in range(len(rows))] if T else []
        occ = [0, 0, 0, 0]
        for r, n in zip(rows, per):
            occ[r] = n
            o = set()
            while len(o) < n:
                o.add((float(np.round(rng.uniform(-0.12, 0.12) * 1024) / 1024), float(np.round(rng.uniform(-0.02, 0.02) * 1024) / 1024), float(np.round(rng.uniform(-0.1, 0.1) * 1024) / 1024)))
            for (ox, oy, oz) in sorted(o):
                pts.append(c + [ox, ROW_OFF[r] + oy, oz])
        qs.append(c); want.append(occ)
    return _case("walk_totals_" + group, group, "exact", dict(kind="walk", rows=want), pts, qs)


# ---------------------------------------------------------------------------------------------------------------- directory
def directory_case():
    """rows whose occupied cells are 2M-1, 2M, 2M+1, 2M+2 empty cells apart (M = the directory's margin), rows with a single occupied cell, and queries every
    cell along each row and the rows next to it: spans that end in the filled margin, in the stale middle of a long gap, and spans that are empty altogether."""
    rng = np.random.default_rng(9)
    M = R.DMARGIN
    pts, qs = [], []
    y = -40 * CELL
    spec = [(2 * M - 1,), (2 * M,), (2 * M + 1,), (2 * M + 2,), (), (2 * M + 1, 2 * M - 1), (0, 2 * M + 2)]
    for gaps in spec:
        cx = -20
        cells = [cx]
        for g in gaps:
            cx += g + 1
            cells.append(cx)
        for c in cells:
            pts += list(_cluster(rng, [c * CELL + 0.4, y + 0.4, 0.0], 7, r=0.25))
        for c in range(cells[0] - M - 3, cells[-1] + M + 4):
            for dy in (0.4, 0.4 - CELL, 0.4 + CELL, 0.4 + 2 * CELL):
                qs.append([c * CELL + 0.37, y + dy, 0.05])
        y += 6 * CELL
    return _case("directory_gaps", "default", "exact", dict(kind="directory", margin=M, gaps=spec), pts, qs)


# ---------------------------------------------------------------------------------------------------------------- ties
def tie_cases():
    out = []
    # a dyadic lattice (0.5 m in x and y, two layers): rings of equal distance around lattice points, cell centres and edge midpoints
    g = np.arange(-3.0, 3.01, 0.5)
    m = np.array([[x, y, z] for z in (0.0, 0.5) for y in g for x in g])
    rng = np.random.default_rng(3)
    m_shuf = m[rng.permutation(len(m))]
    qs = [[x, y, z] for x in (-1.0, -0.75, 0.25, 1.5) for y in (-0.5, 0.25, 1.25) for z in (0.0, 0.25)]
    out.append(_case("ties_lattice", "default", "float", dict(kind="ties"), m_shuf, qs))
    # exact duplicates (an unordered map only: a voxel grid merges them), a tie between the fifth and the sixth, and a tie inside the list
    c = np.array([10.0, 10.0, 1.0])
    dup = [c + [0.25, 0, 0]] * 3 + [c + [0, 0.25, 0]] * 2 + [c + [0, 0, 0.5], c + [0.5, 0, 0], c + [-0.5, 0, 0], c + [0, -0.5, 0], c + [0, 0.5, 0]] + [[-20, -20, 0]]
    out.append(_case("ties_duplicates", "default", "float", dict(kind="ties"), dup, [c, c + [0.25, 0, 0], c + [0.125, 0.125, 0]], states=("init",)))
    c = np.array([-12.0, 6.0, 0.0])
    five_six = [c + [0.125, 0, 0], c + [0, 0.25, 0], c + [0, 0, 0.375], c + [-0.4375, 0, 0], c + [0.5, 0, 0], c + [0, -0.5, 0], c + [0, 0, 0.5], c + [0, 0.5, 0], [30, 0, 0]]
    inside = [c + [40, 0, 0] + o for o in ([0.125, 0, 0], [0, 0.25, 0], [-0.25, 0, 0], [0, 0, 0.25], [0.5, 0, 0], [0, 0.625, 0], [0.75, 0, 0])]
    out.append(_case("ties_fifth_sixth_and_inside", "default", "float", dict(kind="ties"), five_six + inside, [c, c + [40, 0, 0]]))
    # the same two kinds of tie with every point in a leaf of its own (0.4 m and 0.5 m leaves): they survive the voxel grid. The tied pair sits in different rows and
    # different z leaves, the one the walk meets first (lower row) has the HIGHER PCL index (z | y | x) and the higher index in the list below; no other tie in the query
    for group in ("default", "half"):
        pts, qs = [], []
        for k, tie_at in enumerate((4, 2)):
            c = np.array([-12.0 + 24 * k, 6.0, 0.0])
            uniq = [[0.125, 0.125, 0.125], [-0.25, 0.125, 0.125], [0.125, 0.125, -0.4375], [0.625, 0.125, 0.125]]
            pair = [[0.125, 0.625, -0.625], [0.125, -0.625, 0.625]] if tie_at == 4 else [[0.125, 0.375, -0.3125], [0.125, -0.375, 0.3125]]
            rest = uniq if tie_at == 4 else uniq[:2] + [[0.625, 0.125, 0.125], [0.125, 0.125, -0.9375]]
            pts += [c + o for o in pair + rest] + [c + [0.125, 1.125, -1.03125]]
            qs.append(c)
        out.append(_case("ties_one_per_leaf_" + group, group, "float", dict(kind="ties_split"), pts + [[30, -30, 0]], qs))
    g = np.arange(-2.75, 2.76, 0.5)
    m = np.array([[x, y, z] for z in (0.25, 0.75) for y in g for x in g])
    m = m[np.random.default_rng(8).permutation(len(m))]
    qs = [[x, y, z] for x in (-1.25, -0.75, 0.0, 1.5) for y in (-0.25, 0.25, 1.0) for z in (0.25, 0.5)]
    out.append(_case("ties_lattice_half", "half", "float", dict(kind="ties"), m, qs))
    return out


# ---------------------------------------------------------------------------------------------------------------- fits
def line_cases():
    out = []
    s = 0.125
    c0 = np.array([4.0, -2.0, 1.0])

    def five(xs, ys, zs, c=c0):
        return [c + s * np.array([x, y, z]) for x, y, z in zip(xs, ys, zs)]
    far = [[60, 60, 0], [-60, 60, 0]]
    out.append(_case("line_collinear", "default", "exact", dict(kind="line", valid=True), five((-2, -1, 0, 1, 2), (-2, -1, 0, 1, 2), (0, 0, 0, 0, 0)) + far, [c0 + [0.01, 0.02, 0.03]], which="edge"))
    out.append(_case("line_identical", "default", "float", dict(kind="line", valid=False), [c0] * 5 + far, [c0 + [0.1, 0, 0]], which="edge", states=("init",)))
    for tag, h in (("h1", 1.0), ("h0", 0.0), ("h_half", 0.5)):
        # covariance diag(2 h^2, 6, 18) s^2: w2 = 3 w1 exactly -> no factor
        out.append(_case("line_w2_eq_3w1_" + tag, "default", "float", dict(kind="line", valid=False), five((3, -3, 0, 0, 0), (0, 0, 1, 1, -2), (0, 0, h, -h, 0)) + far, [c0 + [0.01, 0, 0]], which="edge"))
    x3 = float(c0[0] + s * 3)
    for tag, xx in (("up", np.nextafter(F32(x3), F32(99))), ("down", np.nextafter(F32(x3), F32(-99)))):
        p = five((3, -3, 0, 0, 0), (0, 0, 1, 1, -2), (0, 0, 1, -1, 0))
        p[0] = np.array([float(xx), p[0][1], p[0][2]])
        out.append(_case("line_w2_3w1_ulp_" + tag, "default", "exact", dict(kind="line", valid=tag == "up"), p + far, [c0 + [0.01, 0, 0]], which="edge"))
    out.append(_case("line_equal_top", "default", "float", dict(kind="line", valid=False), five((2, -2, 0, 0, 0), (0, 0, 2, -2, 0), (0, 0, 0, 0, 0)) + far, [c0 + [0.01, 0, 0]], which="edge"))
    return out


def _lifted_z(side):
    """the float z of the lifted point for which the largest exact residual of the plane through the five points first exceeds (side = +1) / last stays below (-1) 0.2"""
    base = _plane_pts()

    def maxres(zf):
        p = base.copy(); p[4, 2] = zf
        ex = R.exact_query(np.vstack([p, [[50, 50, 50]]]).astype(np.float32), p.mean(0).astype(np.float32), True)
        return max(ex["resid"])
    lo, hi = F32(2.0), F32(3.0)
    assert maxres(lo) < 0.2 < maxres(hi)
    while np.nextafter(lo, F32(9)) < hi:
        mid = F32((float(lo) + float(hi)) / 2)
        if maxres(mid) < 0.2:
            lo = mid
        else:
            hi = mid
    return hi if side > 0 else lo


def _lifted_plane(side):
    """the five points with the largest exact residual as close to 0.2 as the floats allow, above (side = +1) or below: the lifted point puts it within a float of z
    (2e-7), the z of three corners — a smaller effect each — is then stepped through its neighbours for the nearest value on the same side"""
    b = _plane_pts(); b[4, 2] = float(_lifted_z(side))
    steps = []
    for j in (1, 2, 3):
        z = [F32(b[j, 2])]
        for _ in range(6):
            z = [np.nextafter(z[0], F32(-9))] + z + [np.nextafter(z[-1], F32(9))]
        steps.append([float(v) for v in z])
    best = None
    for z1 in steps[0]:                          # pre-selection in double (the residual's own error there is 1e-13), the choice is then confirmed by the exact tier
        for z2 in steps[1]:
            for z3 in steps[2]:
                p = b.copy(); p[1, 2], p[2, 2], p[3, 2] = z1, z2, z3
                n, d = R.plane_fit(p)[1:3]
                r = float(np.abs(p @ n + d).max()) - 0.2
                if r * side > 1e-9 and (best is None or abs(r) < best[0]):
                    best = (abs(r), p)
    ex = R.exact_query(np.vstack([best[1], [[50, 50, 50]]]).astype(np.float32), best[1].mean(0).astype(np.float32), True)
    assert ex["dec_fit"] and (max(ex["resid"]) - 0.2) * side > 0
    return best[1]


def _plane_pts():
    return np.array([[5.0, 5.0, 2.0], [5.5, 5.0, 2.0], [5.0, 5.5, 2.0], [5.5, 5.5, 2.0], [5.25, 5.25, 2.0]])


def plane_cases():
    out = []
    far = [[60.0, 60, 0], [-60, 60, 0]]
    c = np.array([20.0, -30.0, 10.0])
    offs = np.array([[0, 0], [0.5, 0], [0, 0.5], [-0.5, 0.25], [0.25, -0.5]])
    p = [c + [ox, oy, 0.25 * ox - 0.5 * oy] for ox, oy in offs]
    out.append(_case("plane_exact_far", "default", "exact", dict(kind="plane", valid=True), p + far, [c + [0.05, 0.05, 0.3]], which="surf"))
    for tag, side in (("above", 1), ("below", -1)):
        b = _lifted_plane(side)
        out.append(_case("plane_residual_0p2_" + tag, "default", "exact", dict(kind="plane", valid=side < 0, near=5e-8), list(b) + far, [b.mean(0)], which="surf"))
    p0 = [[0.5, 0.25, 0.0], [-0.5, 0.25, 0.0], [0.25, -0.5, 0.0], [-0.25, -0.25, 0.0], [0.125, 0.5, 0.0]]
    out.append(_case("plane_through_origin", "default", "float", dict(kind="plane_degenerate"), p0 + far, [[0.0, 0.0, 0.1]], which="surf"))
    # a plane through the origin with one point lifted by 2e-15: the QR's third pivot is 8.5 eps of the largest — 2.8 times above the reference's rank threshold
    # (eps * 3 * maxpivot), 3.5 times below ten times that. The pivot is the lifted coordinate carried through two reflections (relative error of a few eps), so
    # the rank is 3 in any correct evaluation; the plane is then z = 0 with residuals of 1e-16 (accepted), while rank 2 gives d = 2.4 and residuals far above 0.2.
    # The fit itself is undecided (condition number 1e15): only the kind is compared, bit for bit (kind_by_rule).
    pz = [list(v) for v in p0]; pz[4][2] = 2e-15
    out.append(_case("plane_pivot_8eps", "default", "float", dict(kind="plane_pivot"), pz + far, [[0.0, 0.0, 0.1]], which="surf", states=("init",), kind_by_rule=True))
    out.append(_case("plane_collinear", "default", "float", dict(kind="plane_degenerate"), [c + [t, 2 * t, -t] for t in (-0.25, -0.125, 0, 0.125, 0.25)] + far, [c], which="surf"))
    out.append(_case("plane_identical", "default", "float", dict(kind="plane_degenerate"), [c] * 5 + far, [c + [0.1, 0, 0]], which="surf", states=("init",)))
    return out


# ---------------------------------------------------------------------------------------------------------------- bulk and launch edges
def random_case(group, seed=21, n_map=3000, n_q=257, name="random"):
    """a street-like cloud (ground, two walls, poles) with a pose that is not dyadic; 257 queries = one more than a block"""
    rng = np.random.default_rng(seed)
    n3 = n_map // 3
    ground = np.column_stack([rng.uniform(-14, 14, n3), rng.uniform(-14, 14, n3), rng.normal(-1.5, 0.02, n3)])
    wall = np.column_stack([rng.uniform(-14, 14, n3), np.where(rng.random(n3) < 0.5, -9.0, 9.0) + rng.normal(0, 0.02, n3), rng.uniform(-1.5, 2.5, n3)])
    k = n_map - 2 * n3
    poles = np.column_stack([np.repeat(rng.uniform(-12, 12, 12), (k + 11) // 12)[:k], np.repeat(rng.uniform(-8, 8, 12), (k + 11) // 12)[:k], rng.uniform(-1.5, 3.0, k)]) + rng.normal(0, 0.01, (k, 3))
    m = np.vstack([ground, wall, poles])
    m = m[rng.permutation(len(m))]
    ang = 0.3
    pose = np.array([0.02, -0.03, np.sin(ang / 2), 0, 0.37, -0.21, 0.11]); pose[3] = np.sqrt(1 - (pose[:3] ** 2).sum())
    src = m[rng.choice(len(m), n_q, replace=False)] + rng.normal(0, 0.05, (n_q, 3))
    Rm = _rot(pose)
    q = (src - pose[4:]) @ Rm                      # R^T (p - t): the queries land next to map points
    return _case(name + "_" + group, group, "exact", dict(kind="bulk"), m, q, pose=pose)


def _rot(pose):
    x, y, z, w = pose[:4]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def small_map_cases():
    """maps of 4, 5 and 6 points (three streams of one batch, each with its own pose)"""
    out = []
    base = np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [-0.3, 0.0, 0.1], [0.0, -0.15, 0.0], [0.2, 0.2, 0.05], [0.05, -0.3, -0.1]])
    poses = (IDENT, np.array([0, 0, np.sin(0.2), np.cos(0.2), 1.0, -2.0, 0.5]), np.array([0, np.sin(-0.1), 0, np.cos(-0.1), -3.0, 0.25, 0.0]))
    for n, pose in zip((4, 5, 6), poses):
        c = np.array([3.0 * n, -2.0 * n, 0.0])
        q_world = c + np.array([[0.01, 0.02, 0.0], [0.3, 0.0, 0.0]])
        q = (q_world - pose[4:]) @ _rot(pose)
        out.append(_case("map_size_%d" % n, "tiny", "exact", dict(kind="map_size", n=n), base[:n] + c, q, pose=pose))
    return out


LEAVES["tiny"] = LEAVES["default"]
QUERY_COUNTS = (0, 1, 255, 256, 257)


def all_cases():
    cases = gate_cases() + [walk_case("default"), directory_case()] + tie_cases() + line_cases() + plane_cases() + [random_case("default")]
    cases += [walk_case("small"), random_case("small", seed=22, n_map=2500, n_q=200)]
    cases += small_map_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


# ---------------------------------------------------------------------------------------------------------------- targets
def check_target(case):
    """assert, on the CPU, that the case hits what it was designed for"""
    t = case["target"]; m = case["map"][:, :3]; leaf_e, leaf_s = LEAVES[case["group"]]
    q = R.transform(case["pose"], case["q"][:, :3])
    kind = t["kind"]
    if kind == "gate5":
        idx, d2 = R.knn5(m, q[0])
        assert (d2[4] < F32(1.0)) == t["passes"] and (d2[:5] == d2[0]).all()
        if not t["passes"]:
            assert d2[4] >= F32(1.0)
        if t.get("fits"):
            nb = m[idx].astype(np.float64)
            assert d2[4] == F32(1.0) and R.line_fit(nb)[0] and R.plane_fit(nb)[0] and R.fit_is_robust(nb, False) and R.fit_is_robust(nb, True)
    elif kind == "radius_edge":
        for leaf in (leaf_e, leaf_s):
            cs = R.cell_shift(leaf)
            for p in q:
                idx, d2 = R.knn5(m, p)
                assert F32(0.98) < d2[4] < F32(1.0)
                fx, fy = (int(R.cell_of(m[idx[4], a], leaf, cs)) for a in (0, 1))
                lo = [int(R.cell_of(F32(p[a]) - F32(0.99), leaf, cs)) for a in (0, 1)]; hi = [int(R.cell_of(F32(p[a]) + F32(0.99), leaf, cs)) for a in (0, 1)]
                assert not (lo[0] <= fx <= hi[0] and lo[1] <= fy <= hi[1]), "a radius of 0.99 must miss the fifth neighbour's cell"
                cylo, nrow, cxlo, cxhi1 = R.query_rows(p, leaf, cs)
                assert cxlo <= fx < cxhi1 and cylo <= fy < cylo + nrow
    elif kind == "ties_split":
        for leaf in (leaf_e,):
            key = np.floor(m * (F32(1.0) / F32(leaf))).astype(np.int64)
            assert len(np.unique(key, axis=0)) == len(m), "one point per leaf"
            cs = R.cell_shift(leaf)
            for p, at in zip(q, (4, 2)):
                d = R.sqdist_f32(m, p); order = np.argsort(d, kind="stable")
                ds = d[order][:6]
                assert ds[at] == ds[at + 1] and len(set(ds.tolist())) == 5, ds
                a, b = order[at], order[at + 1]                     # a: the lower list index = the expected one
                pcl = lambda j: tuple(int(v) for v in key[j][::-1])
                assert pcl(a) < pcl(b)
                if at == 4 or case["group"] == "half":
                    assert int(R.cell_of(m[a, 1], leaf, cs)) > int(R.cell_of(m[b, 1], leaf, cs)), "the walk meets the other one first"
    elif kind == "fifth_between":
        idx, d2 = R.knn5(m, q[0])
        assert F32(1.0) < d2[4] < F32(1.001) * F32(1.001)
        cs = R.cell_shift(leaf_e)
        assert tuple(int(R.cell_of(m[idx[4], a], leaf_e, cs)) for a in (0, 1)) != tuple(int(R.cell_of(q[0, a], leaf_e, cs)) for a in (0, 1))
    elif kind == "boundaries":
        for leaf in (leaf_e, leaf_s):
            cs = R.cell_shift(leaf)
            for axis in (0, 1):
                cq = R.cell_of(q[:, axis], leaf, cs)
                assert {int(v) & 511 for v in cq} >= {511, 0, 1, 510}, "the queries must sit on both sides of the slot wrap at 0, in x and in y"
                cm = R.cell_of(m[:, axis], leaf, cs)
                assert (cm & 511).max() > 500 and (cm & 511).min() < 10
    elif kind == "straddle":
        cs = R.cell_shift(leaf_e)
        lo = [R.query_rows(p, leaf_e, cs)[2] for p in q]
        assert len(set(lo)) > 3
        steps = sum(1 for a, b in zip(lo[::2], lo[2::2]) if a != b)
        assert steps >= 5, "neighbouring floats must start their span in different cells"
    elif kind == "walk":
        for leaf in (leaf_e, leaf_s):
            cs = R.cell_shift(leaf)
            totals = set(); deep = 0
            for p, want in zip(q, t["rows"]):
                got = R.candidates_per_row(m, p, leaf, cs)
                assert sum(got) == sum(want), (got, want)
                totals.add(sum(got))
                if case["group"] == "default":
                    assert len(got) == 4 and got == want, (got, want)
                else:
                    deep = max(deep, len(got))
            assert totals == set(WALK_TOTALS)
            assert case["group"] == "default" or deep > 4, "cells below 2/3 m: the rows past the fourth go through the tail loop"
        if case["group"] == "default":
            pats = {tuple(1 if v else 0 for v in w) for w in t["rows"]}
            assert {(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 0, 0, 1), (0, 0, 0, 1), (1, 0, 0, 0)} <= pats      # empty rows first, in the middle, last
            # the first and the last point of the map (cell-major order) are among some query's five
            cs = R.cell_shift(leaf_e)
            key = R.cell_of(m[:, 1], leaf_e, cs) * (1 << 20) + R.cell_of(m[:, 0], leaf_e, cs)
            first, last = set(np.nonzero(key == key.min())[0]), set(np.nonzero(key == key.max())[0])
            used = set()
            for p in q:
                used |= set(int(v) for v in R.knn5(m, p)[0])
            assert used & first and used & last
    elif kind == "directory":
        cs = R.cell_shift(leaf_e)
        cx = R.cell_of(m[:, 0], leaf_e, cs); cy = R.cell_of(m[:, 1], leaf_e, cs)
        seen = set(); single = 0
        for row in np.unique(cy):
            occ = np.unique(cx[cy == row])
            single += len(occ) == 1
            seen |= {int(b - a - 1) for a, b in zip(occ[:-1], occ[1:])}
        M = t["margin"]
        assert {2 * M - 1, 2 * M, 2 * M + 1, 2 * M + 2} <= seen and single >= 1
        # a row break right before and right after the queried cell: queries that sit in the first and in the last occupied cell of a row of the map
        qx = R.cell_of(q[:, 0], leaf_e, cs); qy = R.cell_of(q[:, 1], leaf_e, cs)
        before = after = 0
        for row in np.unique(cy):
            occ = np.unique(cx[cy == row])
            before += int(((qy == row) & (qx == occ[0])).sum()); after += int(((qy == row) & (qx == occ[-1])).sum())
        assert before >= 7 and after >= 7
        empties = sum(1 for p in q if sum(R.candidates_per_row(m, p, leaf_e, cs)) == 0)
        assert empties > 10, "queries whose whole span is empty"
    elif kind == "ties":
        n_56 = n_in = 0
        for p in q:
            d = np.sort(R.sqdist_f32(m, p))
            n_56 += d[4] == d[5]; n_in += (d[:4] == d[1:5]).any()
        assert n_56 + n_in > 0
        if "fifth_sixth" in case["name"]:
            assert n_56 >= 1 and n_in >= 1
    elif kind == "line":
        idx, d2 = R.knn5(m, q[0])
        assert d2[4] < F32(1.0)
        ok = R.line_fit(m[idx].astype(np.float64))[0]
        assert ok == t["valid"], case["name"]
    elif kind == "plane":
        idx, d2 = R.knn5(m, q[0])
        assert d2[4] < F32(1.0)
        ok = R.plane_fit(m[idx].astype(np.float64))[0]
        assert ok == t["valid"], case["name"]
        ex = R.exact_query(m, q[0], True)
        assert ex["dec_fit"] and ex["valid"] == t["valid"]
        if "near" in t:
            assert abs(max(ex["resid"]) - 0.2) < t["near"]
    elif kind == "plane_degenerate":
        idx, d2 = R.knn5(m, q[0])
        assert d2[4] < F32(1.0)
        ex = R.exact_query(m, q[0], True)
        assert not ex["fit_decided"]
    elif kind == "plane_pivot":
        idx, d2 = R.knn5(m, q[0])
        nb = m[idx].astype(np.float64)
        r = np.abs(np.diag(np.linalg.qr(nb)[1]))
        assert 6 * R.EPS < r.min() / r.max() < 15 * R.EPS
        assert R.plane_fit(nb)[0] and R.colpiv_qr_solve(nb, -np.ones(5))[1] == 3
    elif kind == "map_size":
        assert len(m) == t["n"]
    elif kind == "bulk":
        inside = sum(1 for p in q if R.knn5(m, p)[1][4] < F32(1.0))
        assert inside > 0.8 * len(q)
        assert not np.all(case["pose"] * 1024 == np.round(case["pose"] * 1024)), "a pose that is not dyadic"
    else:
        raise AssertionError(kind)
